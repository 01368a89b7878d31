// k_ivtc.hip -- inverse telecine and the field metrics (include/dsv1_api.h, Inverse telecine; stated in numpy in tests/_ivtc.py):
// tightly packed planar 8-bit frames in, 5n per source, the 4n film frames out.  It takes the deinterlacer's place in the source
// chain: behind the source converter, in front of the noise filter.
//
// Six kernels on the lane's stream, no host synchronisation in between -- every decision is made on the device:
//   k_field_metrics   one sweep over the interior luma rows of every frame: mc0 mc1 mp0 mp1 (row y is a line of parity y & 1 between
//                     two lines of the other parity q, so it serves q's sums).  An item is 16 columns of FM_RUN rows in a running
//                     three-row window: every row of cur is loaded once per item.  Per-thread partial sums, wave reduction, LDS across
//                     the block's waves, one integer atomicAdd per block and metric: exact, whatever the order.
//   k_ivtc_match      per frame: P or C from the metrics (ivtc_match_rule, dsvg_ivtc_rules.h).
//   k_ivtc_dup        D_t: the luma SAD of woven picture t against woven picture t - 1.  No woven clip exists: each row is fetched,
//                     through the match table, from the frame that supplies it -- the stream's last input frame for the row of a first
//                     picture matched P, the stored woven luma for the picture before the call.
//   k_ivtc_pick       per cycle of 5: the picture to drop (ivtc_pick_rule) and the output table: output j takes (frame, match).
//   k_ivtc_weave      a gather: output picture, plane, row -> one of two frames by row parity, copied.
//   k_ivtc_keep       the state a stream carries: its last input frame and the luma of its last woven picture.  A launch of its own
//                     behind everything that reads the old state.
// 16-byte loads and stores where every row involved is 16-byte aligned (decided on the host per launch: uniform); a byte path that
// touches exactly the samples the definition names elsewhere.  Nothing outside the frames, the states and the tables is read or
// written.
#include <algorithm>
#include <vector>
#include "dsvg_host.hpp"
#include "dsvg_pixfmt.h"
#include "dsvg_ivtc_rules.h"

#define IV_THREADS 256
#define FM_RUN 8
#define DUP_ROWS 4

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct IvPlane {
    int W, H, cpr, block0;               // columns of 16 per row, first block of the plane in blockIdx.x
    long long off;                       // the plane inside a frame
};
// one launch's view of a clip: ns sources x nin frames, and each source's state (hist frame, then woven luma), or none
struct IvClip {
    const uint8_t *src;
    const uint8_t *state;                // nullptr: the streams start here
    long long sstride;                   // from one source's state to the next's
    long long fb;
    int W, H, nin, nout, p;
    int fast;                            // luma rows of src and state on the 16-byte path
};

static __device__ __forceinline__ u32x4 iv_ld16(const uint8_t *p) { return *reinterpret_cast<const u32x4 *>(p); }

// v[k] summed over the block and added to dst[k]; every thread of the block calls it
template <int N> static __device__ __forceinline__ void iv_block_add(unsigned (&v)[N], unsigned *dst)
{
    __shared__ unsigned part[IV_THREADS / 64][N];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) {
#pragma unroll
        for (int o = 32; o; o >>= 1) v[k] += __shfl_xor(v[k], o);
        if (lane == 0) part[wv][k] = v[k];
    }
    __syncthreads();
    if (tid < N) {
        unsigned s = 0;
#pragma unroll
        for (int k = 0; k < IV_THREADS / 64; k++) s += part[k][tid];
        if (s) atomicAdd(&dst[tid], s);
    }
}

// how far o lies outside the interval of a and b, where that exceeds nt
static __device__ __forceinline__ unsigned fm_e(int a, int b, int o, int nt)
{
    const int e = max(max(min(a, b) - o, o - max(a, b)), 0);
    return e > nt ? (unsigned)e : 0u;
}
static __device__ __forceinline__ unsigned fm_e16(const u32x4 a, const u32x4 b, const u32x4 o, int nt)
{
    unsigned s = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < 32; k += 8) s += fm_e((int)((a[i] >> k) & 0xffu), (int)((b[i] >> k) & 0xffu), (int)((o[i] >> k) & 0xffu), nt);
    return s;
}

// blockIdx.y = frame (source * nin + t); metrics [frame][4], zeroed before the launch.  prev: one frame per source, pstride apart
__global__ __launch_bounds__(IV_THREADS) void k_field_metrics(const uint8_t *__restrict__ src, const uint8_t *__restrict__ prev, long long pstride,
                                                              long long fb, int W, int H, int nin, int nt, int fast, unsigned *__restrict__ metrics)
{
    const int f = (int)blockIdx.y, s = f / nin, t = f - s * nin;
    const uint8_t *cur = src + (long long)f * fb;
    const uint8_t *prv = t > 0 ? cur - fb : (prev ? prev + (long long)s * pstride : nullptr);
    const int cpr = (W + 15) / 16;
    const long long item = (long long)blockIdx.x * IV_THREADS + (int)threadIdx.x;
    const long long run = item / cpr;
    const int col = (int)(item - run * cpr);
    const long long y0 = 1 + run * FM_RUN;               // interior rows: 1 .. H - 2
    unsigned acc[4] = {0u, 0u, 0u, 0u};
    if (y0 <= H - 2) {
        const int ya = (int)y0, yb = min(ya + FM_RUN - 1, H - 2);
        const int x0 = 16 * col, n = min(16, W - x0);
        if (fast) {
            u32x4 a = iv_ld16(cur + (long long)(ya - 1) * W + x0), m = iv_ld16(cur + (long long)ya * W + x0);
            for (int y = ya; y <= yb; y++) {
                const u32x4 b = iv_ld16(cur + (long long)(y + 1) * W + x0);
                const unsigned ec = fm_e16(a, b, m, nt);
                const unsigned ep = prv ? fm_e16(a, b, iv_ld16(prv + (long long)y * W + x0), nt) : 0u;
                if (y & 1) { acc[0] += ec; acc[2] += ep; } else { acc[1] += ec; acc[3] += ep; }
                a = m; m = b;
            }
        } else {
            for (int y = ya; y <= yb; y++) {
                const uint8_t *ra = cur + (long long)(y - 1) * W + x0, *rm = ra + W, *rb = rm + W;
                const uint8_t *rp = prv ? prv + (long long)y * W + x0 : nullptr;
                unsigned ec = 0, ep = 0;
                for (int k = 0; k < n; k++) {
                    ec += fm_e(ra[k], rb[k], rm[k], nt);
                    if (rp) ep += fm_e(ra[k], rb[k], rp[k], nt);
                }
                if (y & 1) { acc[0] += ec; acc[2] += ep; } else { acc[1] += ec; acc[3] += ep; }
            }
        }
    }
    iv_block_add<4>(acc, metrics + (long long)f * 4);
}

__global__ void k_ivtc_match(const unsigned *__restrict__ metrics, int nin, int total, int has_state, int p, uint8_t *__restrict__ match)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= total) return;
    const int t = i % nin;
    match[i] = (uint8_t)ivtc_match_rule(metrics + (long long)i * 4, t > 0 || has_state, p);
}

// the frame that supplies row y of a plane of H rows in the picture woven from frame t with match m.  src_s: the source's frames of
// this call; hist: its last frame of the call before (read only for t == 0 matched P, which the match rule gives only where it exists)
static __device__ __forceinline__ const uint8_t *iv_row_frame(const uint8_t *src_s, const uint8_t *hist, long long fb, int t, int m, int y, int p, int H)
{
    const uint8_t *cur = src_s + (long long)t * fb;
    if (H == 1 || (y & 1) == p || m != IVTC_MATCH_P) return cur;
    return t > 0 ? cur - fb : hist;
}

static __device__ __forceinline__ unsigned iv_sad16(const u32x4 a, const u32x4 b)
{
    unsigned s = __builtin_amdgcn_sad_u8(a.x, b.x, 0u);
    s = __builtin_amdgcn_sad_u8(a.y, b.y, s);
    s = __builtin_amdgcn_sad_u8(a.z, b.z, s);
    return __builtin_amdgcn_sad_u8(a.w, b.w, s);
}

// blockIdx.y = frame; D [frame], zeroed before the launch
__global__ __launch_bounds__(IV_THREADS) void k_ivtc_dup(const IvClip C, const uint8_t *__restrict__ match, unsigned *__restrict__ D)
{
    const int f = (int)blockIdx.y, s = f / C.nin, t = f - s * C.nin;
    const uint8_t *src_s = C.src + (long long)s * C.nin * C.fb;
    const uint8_t *hist = C.state ? C.state + (long long)s * C.sstride : nullptr;
    if (t == 0 && !hist) {                               // a stream's first picture (uniform over the block)
        if (blockIdx.x == 0 && threadIdx.x == 0) D[f] = 0xffffffffu;
        return;
    }
    const int W = C.W, H = C.H, cpr = (W + 15) / 16;
    const long long item = (long long)blockIdx.x * IV_THREADS + (int)threadIdx.x;
    const long long rg = item / cpr;
    const int col = (int)(item - rg * cpr);
    const int x0 = 16 * col, n = min(16, W - x0);
    const int m1 = match[f], m0 = t > 0 ? match[f - 1] : 0;
    unsigned acc[1] = {0u};
    for (int r = 0; r < DUP_ROWS; r++) {
        const long long yy = rg * DUP_ROWS + r;
        if (yy >= H) break;
        const int y = (int)yy;
        const long long ro = (long long)y * W + x0;
        const uint8_t *a = iv_row_frame(src_s, hist, C.fb, t, m1, y, C.p, H) + ro;
        const uint8_t *b = t > 0 ? iv_row_frame(src_s, hist, C.fb, t - 1, m0, y, C.p, H) + ro : hist + C.fb + ro;
        if (C.fast) {
            acc[0] += iv_sad16(iv_ld16(a), iv_ld16(b));
        } else {
            for (int k = 0; k < n; k++) acc[0] += (unsigned)abs((int)a[k] - (int)b[k]);
        }
    }
    iv_block_add<1>(acc, D + f);
}

// per source and cycle: drop [source][cycle]; tab [source][nout]: (frame << 1) | match of every output picture
__global__ void k_ivtc_pick(const unsigned *__restrict__ D, const uint8_t *__restrict__ match, int nin, int nout, int total, uint8_t *__restrict__ drop,
                            int *__restrict__ tab)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= total) return;
    const int ncyc = nin / IVTC_CYCLE, s = i / ncyc, c = i - s * ncyc;
    const long long f0 = (long long)s * nin + IVTC_CYCLE * c;
    const int k = ivtc_pick_rule(D + f0);
    drop[i] = (uint8_t)k;
    int j = 0;
    for (int t = 0; t < IVTC_CYCLE; t++) {
        if (t == k) continue;
        tab[(long long)s * nout + 4 * c + j] = ((IVTC_CYCLE * c + t) << 1) | (int)match[f0 + t];
        j++;
    }
}

struct IvWeave {
    IvPlane pl[3];
    int fastp[3];                        // the plane's rows on the 16-byte path, in src, state and dst
};

// blockIdx.y = output picture (source * nout + j)
__global__ __launch_bounds__(IV_THREADS) void k_ivtc_weave(const IvClip C, const IvWeave G, const int *__restrict__ tab, uint8_t *__restrict__ dst)
{
    const int bx = (int)blockIdx.x;
    const int pi = bx >= G.pl[2].block0 ? 2 : (bx >= G.pl[1].block0 ? 1 : 0);
    const IvPlane &L = G.pl[pi];
    const long long item = (long long)(bx - L.block0) * IV_THREADS + (int)threadIdx.x;
    const long long yy = item / L.cpr;
    if (yy >= L.H) return;
    const int y = (int)yy, col = (int)(item - yy * L.cpr);
    const int o = (int)blockIdx.y, s = o / C.nout;
    const int e = tab[o], t = e >> 1, m = e & 1;
    const uint8_t *src_s = C.src + (long long)s * C.nin * C.fb;
    const uint8_t *hist = C.state ? C.state + (long long)s * C.sstride : nullptr;
    const int x0 = 16 * col, n = min(16, L.W - x0);
    const long long ro = L.off + (long long)y * L.W + x0;
    const uint8_t *from = iv_row_frame(src_s, hist, C.fb, t, m, y, C.p, L.H) + ro;
    uint8_t *to = dst + (long long)o * C.fb + ro;
    if (G.fastp[pi]) {
        *reinterpret_cast<u32x4 *>(to) = iv_ld16(from);
    } else {
        for (int k = 0; k < n; k++) to[k] = from[k];
    }
}

// blockIdx.y = source; blockIdx.x: first the chunks of 16 bytes of the last input frame, from block wov0 on the woven luma's items.
// out: the states written (ostride apart); fast_f / fast_w: 16-byte copies of the frame / of the luma rows
__global__ __launch_bounds__(IV_THREADS) void k_ivtc_keep(const IvClip C, const uint8_t *__restrict__ match, uint8_t *__restrict__ out, long long ostride,
                                                          int wov0, int fast_f, int fast_w)
{
    const int s = (int)blockIdx.y, t = C.nin - 1;
    const uint8_t *src_s = C.src + (long long)s * C.nin * C.fb;
    uint8_t *st = out + (long long)s * ostride;
    if ((int)blockIdx.x < wov0) {
        const long long b0 = ((long long)blockIdx.x * IV_THREADS + (int)threadIdx.x) * 16;
        if (b0 >= C.fb) return;
        const uint8_t *from = src_s + (long long)t * C.fb + b0;
        if (fast_f) {                                    // (fb is then a multiple of 16)
            *reinterpret_cast<u32x4 *>(st + b0) = iv_ld16(from);
        } else {
            const int n = (int)min(16LL, C.fb - b0);
            for (int k = 0; k < n; k++) st[b0 + k] = from[k];
        }
        return;
    }
    const int W = C.W, H = C.H, cpr = (W + 15) / 16;
    const long long item = (long long)((int)blockIdx.x - wov0) * IV_THREADS + (int)threadIdx.x;
    const long long yy = item / cpr;
    if (yy >= H) return;
    const int y = (int)yy, col = (int)(item - yy * cpr);
    const int x0 = 16 * col, n = min(16, W - x0);
    const long long ro = (long long)y * W + x0;
    // (nin >= 5: the frame before the last one is in the clip, the old state is not read)
    const uint8_t *from = iv_row_frame(src_s, nullptr, C.fb, t, match[(long long)s * C.nin + t], y, C.p, H) + ro;
    uint8_t *to = st + C.fb + ro;
    if (fast_w) {
        *reinterpret_cast<u32x4 *>(to) = iv_ld16(from);
    } else {
        for (int k = 0; k < n; k++) to[k] = from[k];
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct dsvg_ivtc {
    int device = 0, nsrc = 0, nin = 0, nout = 0, p = 0, nt = 0, W = 0, H = 0;
    IvPlane pl[3];
    int nblocks = 0, fm_blocks = 0, dup_blocks = 0, keep_f = 0, keep_w = 0;
    size_t fb = 0, sb = 0;               // frame bytes; from one source's state to the next's (session states: padded to 256)
    uint8_t *state = nullptr;            // [nsrc] states
    uint8_t *work = nullptr;             // the tables below, one allocation
    unsigned *metrics = nullptr, *D = nullptr;
    int *tab = nullptr;
    uint8_t *match = nullptr, *drop = nullptr;
    std::vector<unsigned char> valid;    // per source: state holds one
};

extern "C" int dsv1_ivtc_valid(const dsv1_ivtc *iv);

static inline bool al16(uintptr_t m) { return !(m & 15); }

// the grids of one luma of W x H: the metrics', the SAD's, the woven luma's; 0 where the geometry is too large for an int grid
static int iv_luma_grids(int W, int H, int *fm, int *dup, int *wov)
{
    const long long cpr = (W + 15) / 16;
    const long long runs = H >= 3 ? (H - 2 + FM_RUN - 1) / FM_RUN : 0;
    const long long a = (runs * cpr + IV_THREADS - 1) / IV_THREADS, b = (((long long)H + DUP_ROWS - 1) / DUP_ROWS * cpr + IV_THREADS - 1) / IV_THREADS;
    const long long c = ((long long)H * cpr + IV_THREADS - 1) / IV_THREADS;
    if (a > INT_MAX / IV_THREADS || b > INT_MAX / IV_THREADS || c > INT_MAX / IV_THREADS) return 0;
    *fm = (int)a; *dup = (int)b; *wov = (int)c;
    return 1;
}

// the sums are uint32: 255 * W * H must stay below UINT32_MAX, which also marks a first picture's D
static int iv_geom_ok(int w, int h) { return w >= 1 && h >= 1 && (long long)w * h <= 0xffffffffLL / 255 - 1; }

static int fm_launch(hipStream_t st, const uint8_t *src, int W, int H, size_t fb, int nsrc, int nin, const uint8_t *prev, size_t pstride, int nt,
                     int fm_blocks, unsigned *metrics)
{
    HIPCHK(hipMemsetAsync(metrics, 0, sizeof(unsigned) * 4 * (size_t)nsrc * (size_t)nin, st));
    if (!fm_blocks) return DSVG_OK;                      // no interior line: every sum is 0
    const int scap = std::max(1, 65535 / nin);
    for (int s0 = 0; s0 < nsrc; s0 += scap) {
        const int ns = std::min(scap, nsrc - s0);
        const uint8_t *s = src + (size_t)s0 * nin * fb, *p = prev ? prev + (size_t)s0 * pstride : nullptr;
        uintptr_t m = (uintptr_t)s | (uintptr_t)fb | (uintptr_t)W;
        if (p) m |= (uintptr_t)p | (uintptr_t)pstride;
        hipLaunchKernelGGL(k_field_metrics, dim3(fm_blocks, ns * nin), dim3(IV_THREADS), 0, st, s, p, (long long)pstride, (long long)fb, W, H, nin, nt,
                           al16(m) ? 1 : 0, metrics + (size_t)s0 * nin * 4);
    }
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}

// n frames of one stream (prev_dev: the frame before them, or nullptr) -> metrics_dev [n][4] uint32, device memory
extern "C" int dsvg_field_metrics_run(int device, void *stream, const void *src_dev, int w, int h, int subsamp, int n, const void *prev_dev, int nt,
                                      void *metrics_dev)
{
    int fm, dup, wov;
    if (!src_dev || !metrics_dev || n < 1 || nt < 0 || nt > 254 || !iv_geom_ok(w, h)) { dsvg_set_error("bad field metrics arguments"); return DSVG_ERR_ARG; }
    if (dsvg_device_count() <= device || device < 0) { dsvg_set_error("HIP device %d not present", device); (void)hipGetLastError(); return DSVG_ERR_NODEVICE; }
    if (!iv_luma_grids(w, h, &fm, &dup, &wov)) { dsvg_set_error("frame too large for the field metrics' grid"); return DSVG_ERR_UNSUPPORTED; }
    HIPCHK(hipSetDevice(device));
    const size_t fb = (size_t)w * h + 2 * (size_t)rsu(w, fmt_hs(subsamp)) * (size_t)rsu(h, fmt_vs(subsamp));
    // gridDim.y: runs of frames, each run's prev the frame before it
    for (int f0 = 0; f0 < n; f0 += 65535) {
        const int nf = std::min(65535, n - f0);
        const uint8_t *s = (const uint8_t *)src_dev + (size_t)f0 * fb;
        const int rc = fm_launch((hipStream_t)stream, s, w, h, fb, 1, nf, f0 ? s - fb : (const uint8_t *)prev_dev, 0, nt, fm, (unsigned *)metrics_dev + (size_t)f0 * 4);
        if (rc) return rc;
    }
    return DSVG_OK;
}

extern "C" void dsvg_ivtc_destroy(dsvg_ivtc *d)
{
    if (!d) return;
    if (hipSetDevice(d->device) == hipSuccess) {
        if (d->state) (void)hipFree(d->state);
        if (d->work) (void)hipFree(d->work);
    }
    (void)hipGetLastError();
    delete d;
}

static int ivtc_alloc(dsvg_ivtc *d, int with_state)
{
    const size_t F = (size_t)d->nsrc * d->nin, O = (size_t)d->nsrc * d->nout, Cy = (size_t)d->nsrc * (d->nin / IVTC_CYCLE);
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipMalloc((void **)&d->work, sizeof(unsigned) * 5 * F + sizeof(int) * O + F + Cy + 256));
    d->metrics = (unsigned *)d->work;
    d->D = d->metrics + 4 * F;
    d->tab = (int *)(d->D + F);
    d->match = (uint8_t *)(d->tab + O);
    d->drop = d->match + F;
    if (with_state) HIPCHK(hipMalloc((void **)&d->state, d->sb * (size_t)d->nsrc + 256));
    return DSVG_OK;
}

// nin: the frames per source every call brings (a multiple of 5)
extern "C" int dsvg_ivtc_create(dsvg_ivtc **out, int device, int w, int h, int subsamp, const dsv1_ivtc *iv, int nsrc, int nin, int with_state)
{
    if (!out || nsrc < 1 || nin < IVTC_CYCLE || nin % IVTC_CYCLE || !dsv1_ivtc_valid(iv) || !iv_geom_ok(w, h)) { dsvg_set_error("bad inverse telecine arguments"); return DSVG_ERR_ARG; }
    *out = nullptr;
    if (dsvg_device_count() <= device || device < 0) { dsvg_set_error("HIP device %d not present", device); (void)hipGetLastError(); return DSVG_ERR_NODEVICE; }
    if (nin > 65535 || (long long)nsrc * nin > INT_MAX / 8) { dsvg_set_error("too many frames for one inverse telecine call"); return DSVG_ERR_UNSUPPORTED; }
    dsvg_ivtc *d = new dsvg_ivtc();
    d->device = device; d->nsrc = nsrc; d->nin = nin; d->nout = nin / IVTC_CYCLE * 4;
    d->p = iv->tff ? 0 : 1; d->nt = iv->nt; d->W = w; d->H = h;
    d->valid.assign((size_t)nsrc, 0);
    const int cw = rsu(w, fmt_hs(subsamp)), ch = rsu(h, fmt_vs(subsamp));
    long long blocks = 0, off = 0;
    for (int k = 0; k < 3; k++) {
        IvPlane &L = d->pl[k];
        L.W = k ? cw : w; L.H = k ? ch : h;
        L.cpr = (L.W + 15) / 16;
        L.block0 = (int)blocks;
        L.off = off;
        off += (long long)L.W * L.H;
        blocks += ((long long)L.H * L.cpr + IV_THREADS - 1) / IV_THREADS;
        // (the kernels' item index, block * IV_THREADS + thread, stays far inside a long long; the grid is an int)
        if (blocks > INT_MAX / IV_THREADS) { delete d; dsvg_set_error("frame too large for the inverse telecine's grid"); return DSVG_ERR_UNSUPPORTED; }
    }
    d->nblocks = (int)blocks;
    d->fb = (size_t)off;
    d->keep_f = (int)((off + 16LL * IV_THREADS - 1) / (16LL * IV_THREADS));
    if (!iv_luma_grids(w, h, &d->fm_blocks, &d->dup_blocks, &d->keep_w)) { delete d; dsvg_set_error("frame too large for the inverse telecine's grid"); return DSVG_ERR_UNSUPPORTED; }
    d->sb = (d->fb + (size_t)w * h + 255) & ~(size_t)255;
    const int rc = ivtc_alloc(d, with_state);
    if (rc) { dsvg_ivtc_destroy(d); return rc; }
    *out = d;
    return DSVG_OK;
}

// sources s0 .. s0 + ns - 1 (all with a state, sin, or all without: nullptr) through the five kernels; sout (or nullptr): the states to write
static int iv_launch(dsvg_ivtc *d, hipStream_t st, const uint8_t *src, int s0, int ns, const uint8_t *sin, size_t istride, uint8_t *sout, size_t ostride, uint8_t *dst)
{
    const size_t fb = d->fb;
    const int nin = d->nin, nout = d->nout, ncyc = nin / IVTC_CYCLE;
    unsigned *metrics = d->metrics + (size_t)s0 * nin * 4, *D = d->D + (size_t)s0 * nin;
    uint8_t *match = d->match + (size_t)s0 * nin, *drop = d->drop + (size_t)s0 * ncyc;
    int *tab = d->tab + (size_t)s0 * nout;
    int rc;
    if ((rc = fm_launch(st, src, d->W, d->H, fb, ns, nin, sin, istride, d->nt, d->fm_blocks, metrics))) return rc;
    hipLaunchKernelGGL(k_ivtc_match, dim3((ns * nin + 255) / 256), dim3(256), 0, st, metrics, nin, ns * nin, sin ? 1 : 0, d->p, match);
    HIPCHK(hipMemsetAsync(D, 0, sizeof(unsigned) * (size_t)ns * nin, st));
    const int scap = 65535 / nin;
    // the clip of the group of sources that starts at g0, and what its alignment rests on
    auto group = [&](int g0, uintptr_t *m) {
        IvClip C;
        C.src = src + (size_t)g0 * nin * fb;
        C.state = sin ? sin + (size_t)g0 * istride : nullptr;
        C.sstride = (long long)istride; C.fb = (long long)fb;
        C.W = d->W; C.H = d->H; C.nin = nin; C.nout = nout; C.p = d->p;
        *m = (uintptr_t)C.src | (uintptr_t)fb;
        if (C.state) *m |= (uintptr_t)C.state | (uintptr_t)istride;
        C.fast = al16(*m | (uintptr_t)d->W) ? 1 : 0;
        return C;
    };
    uintptr_t m;
    for (int g0 = 0; g0 < ns; g0 += scap) {              // gridDim.y: groups of sources
        const int g = std::min(scap, ns - g0);
        const IvClip C = group(g0, &m);
        hipLaunchKernelGGL(k_ivtc_dup, dim3(d->dup_blocks, g * nin), dim3(IV_THREADS), 0, st, C, match + (size_t)g0 * nin, D + (size_t)g0 * nin);
    }
    hipLaunchKernelGGL(k_ivtc_pick, dim3((ns * ncyc + 255) / 256), dim3(256), 0, st, D, match, nin, nout, ns * ncyc, drop, tab);
    for (int g0 = 0; g0 < ns; g0 += scap) {
        const int g = std::min(scap, ns - g0);
        const IvClip C = group(g0, &m);
        uint8_t *o = dst + (size_t)g0 * nout * fb;
        m |= (uintptr_t)o;
        IvWeave G;
        for (int k = 0; k < 3; k++) {
            G.pl[k] = d->pl[k];
            G.fastp[k] = al16(m | (uintptr_t)d->pl[k].off | (uintptr_t)d->pl[k].W) ? 1 : 0;
        }
        hipLaunchKernelGGL(k_ivtc_weave, dim3(d->nblocks, g * nout), dim3(IV_THREADS), 0, st, C, G, tab + (size_t)g0 * nout, o);
        if (sout) {                                      // behind the weave, which may read the state this overwrites
            uint8_t *so = sout + (size_t)g0 * ostride;
            const uintptr_t mo = (uintptr_t)C.src | (uintptr_t)fb | (uintptr_t)so | (uintptr_t)ostride;
            hipLaunchKernelGGL(k_ivtc_keep, dim3(d->keep_f + d->keep_w, g), dim3(IV_THREADS), 0, st, C, match + (size_t)g0 * nin, so, (long long)ostride,
                               d->keep_f, al16(mo) ? 1 : 0, al16(mo | (uintptr_t)d->W) ? 1 : 0);
        }
    }
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}

// a session's call: nin frames of each of the nsrc sources -> nout pictures each; the states are read and then refreshed
extern "C" int dsvg_ivtc_run(dsvg_ivtc *d, void *stream, const void *src_dev, void *dst_dev)
{
    if (!d || !d->state || !src_dev || !dst_dev) { dsvg_set_error("bad inverse telecine arguments"); return DSVG_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(d->device));
    const uint8_t *src = (const uint8_t *)src_dev;
    uint8_t *dst = (uint8_t *)dst_dev;
    for (int s0 = 0; s0 < d->nsrc;) {                    // sources with and without a state: runs of either kind
        int s1 = s0 + 1;
        while (s1 < d->nsrc && d->valid[(size_t)s1] == d->valid[(size_t)s0]) s1++;
        uint8_t *state = d->state + (size_t)s0 * d->sb;
        const int rc = iv_launch(d, st, src + (size_t)s0 * d->nin * d->fb, s0, s1 - s0, d->valid[(size_t)s0] ? state : nullptr, d->sb, state, d->sb,
                                 dst + (size_t)s0 * d->nout * d->fb);
        if (rc) return rc;
        s0 = s1;
    }
    for (int s = 0; s < d->nsrc; s++) d->valid[(size_t)s] = 1;
    return DSVG_OK;
}

// the standalone pass over one stream's nin frames: explicit states (fb + W * H bytes, device memory, either may be nullptr, they may be
// the same), none kept
extern "C" int dsvg_ivtc_clip(dsvg_ivtc *d, void *stream, const void *src_dev, const void *state_in_dev, void *state_out_dev, void *dst_dev)
{
    if (!d || d->nsrc != 1 || !src_dev || !dst_dev) { dsvg_set_error("bad inverse telecine arguments"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(d->device));
    return iv_launch(d, (hipStream_t)stream, (const uint8_t *)src_dev, 0, 1, (const uint8_t *)state_in_dev, 0, (uint8_t *)state_out_dev, 0, (uint8_t *)dst_dev);
}

// where the last call's decisions lie in device memory: match [nsrc][nin], drop [nsrc][nin / 5]
extern "C" void dsvg_ivtc_tables(const dsvg_ivtc *d, const void **match_dev, const void **drop_dev)
{
    *match_dev = d->match;
    *drop_dev = d->drop;
}

extern "C" int dsvg_ivtc_reset(dsvg_ivtc *d, int source)
{
    if (!d || source < -1 || source >= d->nsrc) return DSVG_ERR_ARG;
    for (int s = 0; s < d->nsrc; s++)
        if (source < 0 || s == source) d->valid[(size_t)s] = 0;
    return DSVG_OK;
}
