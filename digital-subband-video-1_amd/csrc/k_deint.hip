// k_deint.hip -- the deinterlacer (include/dsv1_api.h, Deinterlacing; stated in numpy in tests/_deint.py): tightly packed planar
// 8-bit frames in, the same out, at frame rate (n -> n) or field rate (n -> 2n).  A streaming stencil in front of the scaler / the
// frame load, behind the source converter.
//
// One launch deinterlaces a clip of one or more sources: blockIdx.y = output picture, blockIdx.x = 256 ITEMS of one plane (the planes'
// blocks one after the other, so a block's plane is uniform).  An output picture keeps the lines of one parity q and makes the
// others; rows come in PAIRS (2i, 2i + 1), one kept and one made.  An item is 16 columns of DI_RUN consecutive pairs: the kept row
// below a made line is the kept row above the next one, so inside a run every kept row of `cur` and `prv` is loaded once, serves
// as e of one line and as c of the next, and is stored from the registers it was loaded into.
// The 16-byte path: rows as one aligned 16-byte load and the two neighbour dwords; the byte windows of the five directions come out
// of them with v_alignbyte_b32, S(j) is one v_sad_u8 of two windows masked to three bytes, P(j) reads the windows' middle bytes, the
// clamp is one v_med3_i32.  It needs every row of the plane 16-byte aligned in `cur`, `prv` and the output (decided on the host per
// launch and plane: uniform) and an item whose columns x - 3 .. x + 19 lie inside the row.  Everything else -- a plane that is not
// aligned, the first and the last item of a row (the column clamp), row tails -- takes the byte path, which loads exactly the
// samples the definition names: nothing outside the frames is read or written.
#include <algorithm>
#include <vector>
#include "dsvg_host.hpp"
#include "dsvg_pixfmt.h"

#define DI_THREADS 256
#define DI_RUN 4

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct DiPlane {
    int W, H, cpr, block0;               // columns of 16 per row, first block of the plane in blockIdx.x
    int fast, pad;                       // every row on the 16-byte path
    long long off;                       // the plane inside a frame
};
struct DiParams {
    DiPlane pl[3];
    long long fb, pstride;               // frame bytes; from one source's `prev` frame to the next's
    int nin, nout, field, p;             // input / output pictures per source, FIELD mode, the first field's parity
};

// the direction search's pick among S(-2..2) / P(-2..2), all by value: selects on registers, nothing indexed by the winner
static __device__ __forceinline__ int di_pick(int sm2, int sm1, int s0, int s1, int s2, int pm2, int pm1, int p0, int p1, int p2)
{
    int best = s0 - 1, sp = p0;
    const bool a = sm1 < best;
    best = a ? sm1 : best; sp = a ? pm1 : sp;
    const bool b = a & (sm2 < best);
    best = b ? sm2 : best; sp = b ? pm2 : sp;
    const bool c = s1 < best;
    best = c ? s1 : best; sp = c ? p1 : sp;
    const bool d = c & (s2 < best);
    return d ? p2 : sp;
}
// the motion bound: a = prv[y][x], b = cur[y][x], pu / pd = prv[up][x] / prv[dn][x], c0 / e0 = cur[up][x] / cur[dn][x]
static __device__ __forceinline__ int di_bound(int sp, int a, int b, int pu, int pd, int c0, int e0, int second)
{
    const int tp = second ? b : (a + b) >> 1;
    const int td0 = abs(a - b) >> 1, td1 = (abs(pu - c0) + abs(pd - e0)) >> 1;
    const int d = max(td0, td1);
    return min(max(sp, tp - d), tp + d);                 // (v_med3_i32)
}

// byte path: one made sample; cu / ce: the rows above and below in cur, cm: its own; pu / pe / pm: the same rows of prv (pm == nullptr: none)
static __device__ int di_sample(const uint8_t *cu, const uint8_t *ce, const uint8_t *cm, const uint8_t *pu, const uint8_t *pe, const uint8_t *pm,
                                int W, int x, int second)
{
    int S[5], P[5];
#pragma unroll
    for (int j = -2; j <= 2; j++) {
        int s = 0;
#pragma unroll
        for (int k = -1; k <= 1; k++) s += abs((int)cu[min(max(x + k + j, 0), W - 1)] - (int)ce[min(max(x + k - j, 0), W - 1)]);
        S[j + 2] = s;
        P[j + 2] = ((int)cu[min(max(x + j, 0), W - 1)] + (int)ce[min(max(x - j, 0), W - 1)]) >> 1;
    }
    const int sp = di_pick(S[0], S[1], S[2], S[3], S[4], P[0], P[1], P[2], P[3], P[4]);
    if (!pm) return sp;
    return di_bound(sp, pm[x], cm[x], pu[x], pe[x], cu[x], ce[x], second);
}

// 16-byte path: a row's 16 bytes at x0 with the dwords left and right of them
static __device__ __forceinline__ void di_load6(const uint8_t *row, unsigned *r6)
{
    const u32x4 b = *reinterpret_cast<const u32x4 *>(row);
    r6[0] = *reinterpret_cast<const unsigned *>(row - 4);
    r6[1] = b.x; r6[2] = b.y; r6[3] = b.z; r6[4] = b.w;
    r6[5] = *reinterpret_cast<const unsigned *>(row + 16);
}
static __device__ __forceinline__ u32x4 di_body(const unsigned *r6)
{
    u32x4 v;
    v.x = r6[1]; v.y = r6[2]; v.z = r6[3]; v.w = r6[4];
    return v;
}
// the three bytes at columns p .. p + 2 of the item (p = -3 .. 16; r6[0] holds columns -4 .. -1)
static __device__ __forceinline__ unsigned di_win(const unsigned *r6, int p)
{
    const int o = p + 4, i = o >> 2, sh = o & 3;
    return (sh ? __builtin_amdgcn_alignbyte(r6[i + 1], r6[i], sh) : r6[i]) & 0x00ffffffu;
}
static __device__ __forceinline__ int di_byte(const u32x4 v, int x) { return (int)((v[x >> 2] >> (8 * (x & 3))) & 0xffu); }

static __device__ __forceinline__ u32x4 di_made16(const unsigned *c6, const unsigned *e6, const u32x4 m, const u32x4 pm, const u32x4 pu, const u32x4 pd,
                                                  bool has_prv, int second)
{
    unsigned cw[20], ew[20];             // window [i]: columns i - 3 .. i - 1
#pragma unroll
    for (int i = 0; i < 20; i++) { cw[i] = di_win(c6, i - 3); ew[i] = di_win(e6, i - 3); }
    u32x4 o = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int x = 0; x < 16; x++) {
        int S[5], P[5];
#pragma unroll
        for (int j = -2; j <= 2; j++) {
            // c columns x - 1 + j .. x + 1 + j: window x + 2 + j, whose middle byte is c[x + j]; e mirrored
            const unsigned a = cw[x + 2 + j], b = ew[x + 2 - j];
            S[j + 2] = (int)__builtin_amdgcn_sad_u8(a, b, 0u);
            P[j + 2] = (int)(((a >> 8) & 0xffu) + ((b >> 8) & 0xffu)) >> 1;
        }
        int r = di_pick(S[0], S[1], S[2], S[3], S[4], P[0], P[1], P[2], P[3], P[4]);
        if (has_prv) r = di_bound(r, di_byte(pm, x), di_byte(m, x), di_byte(pu, x), di_byte(pd, x), (int)((cw[x + 2] >> 8) & 0xffu), (int)((ew[x + 2] >> 8) & 0xffu), second);
        o[x >> 2] |= (unsigned)r << (8 * (x & 3));
    }
    return o;
}

__global__ __launch_bounds__(DI_THREADS) void k_deint(const DiParams P, const uint8_t *__restrict__ src, const uint8_t *__restrict__ prev, uint8_t *__restrict__ dst)
{
    const int bx = blockIdx.x;
    const int pi = bx >= P.pl[2].block0 ? 2 : (bx >= P.pl[1].block0 ? 1 : 0);
    const DiPlane &L = P.pl[pi];
    const int W = L.W, H = L.H, cpr = L.cpr;
    const int item = (bx - L.block0) * DI_THREADS + (int)threadIdx.x;
    const int run = item / cpr, col = item - run * cpr;
    const int npairs = (H + 1) >> 1, i0 = run * DI_RUN;
    if (i0 >= npairs) return;
    // output picture -> source, input frame, which field it keeps
    const int o = blockIdx.y;
    const int s = o / P.nout, jo = o - s * P.nout;
    const int t = P.field ? jo >> 1 : jo;
    const int second = P.field & jo & 1;
    const int q = second ? 1 - P.p : P.p;
    const uint8_t *cur = src + ((long long)s * P.nin + t) * P.fb + L.off;
    const uint8_t *prv = t > 0 ? cur - P.fb : (prev ? prev + (long long)s * P.pstride + L.off : nullptr);
    uint8_t *out = dst + (long long)o * P.fb + L.off;
    const int x0 = 16 * col;
    const int n = min(16, W - x0);
    if (H == 1) {
        for (int i = 0; i < n; i++) out[x0 + i] = cur[x0 + i];
        return;
    }
    const bool has_prv = prv != nullptr;
    if (L.fast && col >= 1 && x0 + 20 <= W) {
        unsigned c6[6], e6[6];
        u32x4 pu = {0u, 0u, 0u, 0u}, pd = pu, pm = pu;
#pragma unroll
        for (int r = 0; r < DI_RUN; r++) {
            const int i = i0 + r;
            if (i >= npairs) break;
            const int y = 2 * i + 1 - q;                 // the made line of the pair (q == 0 and H odd: the last pair has none)
            const int up = y - 1 >= 0 ? y - 1 : y + 1;
            const int dn = y + 1 <= H - 1 ? y + 1 : y - 1;
            if (r == 0) {                                // (later pairs: the row below the line before)
                const int cr = y <= H - 1 ? up : 2 * i;
                di_load6(cur + (long long)cr * W + x0, c6);
                if (has_prv && y <= H - 1) pu = *reinterpret_cast<const u32x4 *>(prv + (long long)cr * W + x0);
            }
            if (y > H - 1) {                             // only the kept row 2i, which is in c6
                *reinterpret_cast<u32x4 *>(out + (long long)(2 * i) * W + x0) = di_body(c6);
                break;
            }
            if (dn != up) {
                di_load6(cur + (long long)dn * W + x0, e6);
                if (has_prv) pd = *reinterpret_cast<const u32x4 *>(prv + (long long)dn * W + x0);
            } else {
#pragma unroll
                for (int k = 0; k < 6; k++) e6[k] = c6[k];
                pd = pu;
            }
            const u32x4 m = *reinterpret_cast<const u32x4 *>(cur + (long long)y * W + x0);
            if (has_prv) pm = *reinterpret_cast<const u32x4 *>(prv + (long long)y * W + x0);
            *reinterpret_cast<u32x4 *>(out + (long long)y * W + x0) = di_made16(c6, e6, m, pm, pu, pd, has_prv, second);
            // the pair's kept row: above the made line (q == 0: always row up) or below it (q == 1: row dn, where it exists)
            if (q == 0) *reinterpret_cast<u32x4 *>(out + (long long)(y - 1) * W + x0) = di_body(c6);
            else if (y + 1 <= H - 1) *reinterpret_cast<u32x4 *>(out + (long long)(y + 1) * W + x0) = di_body(e6);
#pragma unroll
            for (int k = 0; k < 6; k++) c6[k] = e6[k];
            pu = pd;
        }
        return;
    }
    for (int r = 0; r < DI_RUN; r++) {
        const int i = i0 + r;
        if (i >= npairs) break;
        const int y = 2 * i + 1 - q, kept = 2 * i + q;
        if (kept <= H - 1)
            for (int k = 0; k < n; k++) out[(long long)kept * W + x0 + k] = cur[(long long)kept * W + x0 + k];
        if (y > H - 1) continue;
        const int up = y - 1 >= 0 ? y - 1 : y + 1;
        const int dn = y + 1 <= H - 1 ? y + 1 : y - 1;
        const uint8_t *cu = cur + (long long)up * W, *ce = cur + (long long)dn * W, *cm = cur + (long long)y * W;
        const uint8_t *qu = has_prv ? prv + (long long)up * W : nullptr, *qe = has_prv ? prv + (long long)dn * W : nullptr;
        const uint8_t *qm = has_prv ? prv + (long long)y * W : nullptr;
        for (int k = 0; k < n; k++) out[(long long)y * W + x0 + k] = (uint8_t)di_sample(cu, ce, cm, qu, qe, qm, W, x0 + k, second);
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct dsvg_deint {
    int device = 0, mode = 0, tff = 0, nsrc = 0;
    DiParams P;
    int nblocks = 0;
    size_t fb = 0;
    uint8_t *hist = nullptr;             // [nsrc] frames: each source's last input frame
    std::vector<unsigned char> valid;    // per source: hist holds one
};

extern "C" int dsv1_deint_valid(const dsv1_deint *di);

extern "C" void dsvg_deint_destroy(dsvg_deint *d)
{
    if (!d) return;
    if (d->hist && hipSetDevice(d->device) == hipSuccess) (void)hipFree(d->hist);
    (void)hipGetLastError();
    delete d;
}

static int deint_history(dsvg_deint *d)
{
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipMalloc((void **)&d->hist, d->fb * (size_t)d->nsrc + 256));
    return DSVG_OK;
}

extern "C" int dsvg_deint_create(dsvg_deint **out, int device, int w, int h, int subsamp, const dsv1_deint *di, int nsrc, int with_history)
{
    if (!out || w < 1 || h < 1 || nsrc < 1 || !dsv1_deint_valid(di)) { dsvg_set_error("bad deinterlacer arguments"); return DSVG_ERR_ARG; }
    *out = nullptr;
    if (dsvg_device_count() <= device || device < 0) { dsvg_set_error("HIP device %d not present", device); (void)hipGetLastError(); return DSVG_ERR_NODEVICE; }
    dsvg_deint *d = new dsvg_deint();
    d->device = device; d->mode = di->mode; d->tff = di->tff; d->nsrc = nsrc;
    d->valid.assign((size_t)nsrc, 0);
    const int cw = (w + (1 << ((subsamp >> 2) & 3)) - 1) >> ((subsamp >> 2) & 3), ch = (h + (1 << (subsamp & 3)) - 1) >> (subsamp & 3);
    memset(&d->P, 0, sizeof d->P);
    long long blocks = 0, off = 0;
    for (int k = 0; k < 3; k++) {
        DiPlane &L = d->P.pl[k];
        L.W = k ? cw : w; L.H = k ? ch : h;
        L.cpr = (L.W + 15) / 16;
        L.block0 = (int)blocks;
        L.off = off;
        off += (long long)L.W * L.H;
        const long long runs = (((L.H + 1) >> 1) + DI_RUN - 1) / DI_RUN;
        blocks += (runs * L.cpr + DI_THREADS - 1) / DI_THREADS;
        // (the kernel's item index, block * DI_THREADS + thread, is an int)
        if (blocks > INT_MAX / DI_THREADS) { delete d; dsvg_set_error("frame too large for the deinterlacer's grid"); return DSVG_ERR_UNSUPPORTED; }
    }
    d->nblocks = (int)blocks;
    d->fb = (size_t)off;
    d->P.fb = off;
    d->P.field = di->mode == DSV1_DEINT_FIELD;
    d->P.p = di->tff ? 0 : 1;
    const int rc = with_history ? deint_history(d) : DSVG_OK;
    if (rc) { dsvg_deint_destroy(d); return rc; }
    *out = d;
    return DSVG_OK;
}

// nsrc sources x nin frames ([source][frame]) -> nsrc x (nin or 2 nin) pictures; prev: one frame per source, pstride apart, or nullptr
static int di_launch(const dsvg_deint *d, hipStream_t st, const uint8_t *src, int nsrc, int nin, const uint8_t *prev, size_t pstride, uint8_t *dst)
{
    const int per = d->P.field ? 2 : 1;
    const size_t fb = d->fb;
    if (nsrc > 1 && (long long)nin * per > 65535) { dsvg_set_error("too many frames per source for one deinterlacer call"); return DSVG_ERR_UNSUPPORTED; }
    // gridDim.y: a single source's clip goes in runs of frames (each run's `prev` is the frame before it), several sources in groups
    const int fcap = nsrc == 1 ? 65535 / per : nin, scap = nsrc == 1 ? 1 : 65535 / (nin * per);
    for (int s0 = 0; s0 < nsrc; s0 += scap) {
        const int ns = std::min(scap, nsrc - s0);
        for (int f0 = 0; f0 < nin; f0 += fcap) {
            const int nf = std::min(fcap, nin - f0);
            DiParams P = d->P;
            const uint8_t *s = src + ((size_t)s0 * nin + f0) * fb;
            const uint8_t *p = f0 ? s - fb : (prev ? prev + (size_t)s0 * pstride : nullptr);
            uint8_t *o = dst + ((size_t)s0 * nin + f0) * per * fb;
            P.nin = nf; P.nout = nf * per;
            P.pstride = f0 ? 0 : (long long)pstride;
            for (int k = 0; k < 3; k++) {
                const DiPlane &L = P.pl[k];
                uintptr_t m = (uintptr_t)s | (uintptr_t)o | (uintptr_t)fb | (uintptr_t)L.off | (uintptr_t)L.W;
                if (p) m |= (uintptr_t)p | (uintptr_t)P.pstride;
                P.pl[k].fast = L.H > 1 && !(m & 15);
            }
            hipLaunchKernelGGL(k_deint, dim3(d->nblocks, ns * nf * per), dim3(DI_THREADS), 0, st, P, s, p, o);
        }
    }
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}

// a session's call: nin frames of each of the nsrc sources; `prev` is what the deinterlacer kept of the call before, and the call's
// last input frames are kept for the next
extern "C" int dsvg_deint_run(dsvg_deint *d, void *stream, const void *src_dev, int nin, void *dst_dev)
{
    if (!d || !d->hist || !src_dev || !dst_dev || nin < 1) { dsvg_set_error("bad deinterlace arguments"); return DSVG_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(d->device));
    const uint8_t *src = (const uint8_t *)src_dev;
    uint8_t *dst = (uint8_t *)dst_dev;
    const int per = d->P.field ? 2 : 1;
    for (int s0 = 0; s0 < d->nsrc;) {                    // sources with and without a history: runs of either kind
        int s1 = s0 + 1;
        while (s1 < d->nsrc && d->valid[(size_t)s1] == d->valid[(size_t)s0]) s1++;
        const int rc = di_launch(d, st, src + (size_t)s0 * nin * d->fb, s1 - s0, nin, d->valid[(size_t)s0] ? d->hist + (size_t)s0 * d->fb : nullptr, d->fb,
                                 dst + (size_t)s0 * nin * per * d->fb);
        if (rc) return rc;
        s0 = s1;
    }
    for (int s = 0; s < d->nsrc; s++) {
        HIPCHK(hipMemcpyAsync(d->hist + (size_t)s * d->fb, src + ((size_t)s * nin + (nin - 1)) * d->fb, d->fb, hipMemcpyDeviceToDevice, st));
        d->valid[(size_t)s] = 1;
    }
    return DSVG_OK;
}

// the standalone pass: n frames of one stream, `prev` (device, or nullptr) the frame before them; no history is read or kept
extern "C" int dsvg_deint_clip(dsvg_deint *d, void *stream, const void *src_dev, int n, const void *prev_dev, void *dst_dev)
{
    if (!d || !src_dev || !dst_dev || n < 1) { dsvg_set_error("bad deinterlace arguments"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(d->device));
    return di_launch(d, (hipStream_t)stream, (const uint8_t *)src_dev, 1, n, (const uint8_t *)prev_dev, 0, (uint8_t *)dst_dev);
}

extern "C" int dsvg_deint_reset(dsvg_deint *d, int source)
{
    if (!d || source < -1 || source >= d->nsrc) return DSVG_ERR_ARG;
    for (int s = 0; s < d->nsrc; s++)
        if (source < 0 || s == source) d->valid[(size_t)s] = 0;
    return DSVG_OK;
}
