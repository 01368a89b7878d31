// k_denoise.hip -- the temporal noise filter (include/dsv1_api.h, Temporal noise reduction; stated in numpy in tests/_denoise.py):
// tightly packed planar 8-bit pictures in, the same number out.  A motion-adaptive recursion along time in front of the scaler / the
// frame load, behind the source converter and the deinterlacer.
//
// One launch filters a whole clip of one or more sources: blockIdx.y = source, blockIdx.x = 256 ITEMS of one plane (the planes'
// blocks one after the other, so a block's plane is uniform).  The recursion runs along time only and the 3x3 window reads INPUTS
// only, so an item -- 16 columns of DN_ROWS rows -- marches t = 0 .. n - 1 on its own: the filter state S of its samples and the
// window rows of the picture before (its rows and one above and below) stay in registers, every picture is loaded once (the halo
// rows a second time, out of the cache), the output is written once, and the state -- pin, the last input picture, and S -- is read
// at the call's first picture and written at its last.
// The 16-byte path: a window row is one aligned 16-byte load and the two bytes left and right of it, loaded from CLAMPED addresses,
// so the first and the last item of a row and the first and last rows of a plane run the same code as every other; the three-byte
// windows come out of the row with v_perm_b32 (the fourth byte zeroed by the selector), a window's |cur - pin| sum is one v_sad_u8.
// It needs every row of the plane 16-byte aligned in every buffer of the launch (decided on the host per launch and plane: uniform;
// such a plane has no row tails).  Every other plane takes the byte path, which loads exactly the samples the definition names and
// keeps S in the output state between pictures.  Nothing outside the frames and the states is read or written.
// The gain k = 4 + (12 (m - T) + T / 2) / T, clamped to 4 .. 16, is one fma and one conversion: (12 / T) m + (4 - 12 + (T / 2 + 0.5) / T)
// truncated; the exact quotient's fraction is at least 0.5 / T >= 2^-10 away from the next integer and the binary32 error below
// 2^-17 wherever the value lies inside 3 .. 17 (tests/test_denoise_host.py walks every T and m).
#include <algorithm>
#include <vector>
#include "dsvg_host.hpp"
#include "dsvg_pixfmt.h"

#define DN_THREADS 256
#define DN_ROWS 4

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct DnPlane {
    int W, H, cpr, block0;               // columns of 16 per row, first block of the plane in blockIdx.x
    int fast, T;                         // every row on the 16-byte path; the strength
    float ka, kb;                        // the gain's line
    long long off;                       // the plane inside a frame
};
struct DnParams {
    DnPlane pl[3];
    long long fb;                        // frame bytes
    long long pin_in_stride, s_in_stride, pin_out_stride, s_out_stride;  // source to source, bytes
    int n, has_state;                    // pictures per source; pin_in / s_in hold the state the call starts from
};

// S' of one sample: c the input, S the state, m0 the 3x3 SAD of the inputs
static __device__ __forceinline__ int dn_next(int c, int S, int m0, float ka, float kb)
{
    const int pout = (S + 8) >> 4;
    const int m = max(m0, 3 * abs(c - pout));
    const int k = min(max((int)fmaf((float)m, ka, kb), 4), 16);
    return S + (((16 * c - S) * k + 8) >> 4);
}

// 16-byte path: e[0] bits 31:24 = the sample left of the item (clamped), e[1 .. 4] its 16 samples, e[5] bits 7:0 the one right of it
static __device__ __forceinline__ void dn_load_row(const uint8_t *row, int x0, int W, unsigned *e)
{
    const u32x4 b = *reinterpret_cast<const u32x4 *>(row + x0);
    e[0] = (unsigned)row[max(x0 - 1, 0)] << 24;
    e[1] = b.x; e[2] = b.y; e[3] = b.z; e[4] = b.w;
    e[5] = (unsigned)row[min(x0 + 16, W - 1)];
}
// the samples at columns x - 1 .. x + 1 of the item in bits 23:0, bits 31:24 zero
static __device__ __forceinline__ unsigned dn_win(const unsigned *e, int x)
{
    const int o = x + 3, i = o >> 2, sh = o & 3;
    const unsigned sel = 0x0c000000u | ((unsigned)(sh + 2) << 16) | ((unsigned)(sh + 1) << 8) | (unsigned)sh;
    return __builtin_amdgcn_perm(e[i + 1], e[i], sel);
}

__global__ __launch_bounds__(DN_THREADS) void k_denoise(const DnParams P, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                        const uint8_t *__restrict__ pin_in, const uint8_t *__restrict__ s_in,
                                                        uint8_t *__restrict__ pin_out, uint8_t *__restrict__ s_out)
{
    const int bx = blockIdx.x;
    const int pi = bx >= P.pl[2].block0 ? 2 : (bx >= P.pl[1].block0 ? 1 : 0);
    const DnPlane &L = P.pl[pi];
    const int W = L.W, H = L.H, cpr = L.cpr, n = P.n;
    const int item = (bx - L.block0) * DN_THREADS + (int)threadIdx.x;
    const int run = item / cpr, col = item - run * cpr;
    const int y0 = run * DN_ROWS;
    if (y0 >= H) return;
    const long long sidx = blockIdx.y;
    const int x0 = 16 * col;
    const int nc = min(16, W - x0);
    const uint8_t *cur = src + sidx * n * P.fb + L.off;
    uint8_t *out = dst + sidx * n * P.fb + L.off;
    const uint8_t *pi_ = pin_in ? pin_in + sidx * P.pin_in_stride + L.off : nullptr;
    const uint8_t *si_ = s_in ? s_in + sidx * P.s_in_stride + 2 * L.off : nullptr;
    uint8_t *po_ = pin_out + sidx * P.pin_out_stride + L.off;
    uint8_t *so_ = s_out + sidx * P.s_out_stride + 2 * L.off;
    const float ka = L.ka, kb = L.kb;

    if (L.T == 0) {                                      // a copy; the state of such a plane is zeros
        for (int r = 0; r < DN_ROWS && y0 + r < H; r++) {
            const long long o = (long long)(y0 + r) * W + x0;
            if (L.fast) {
                for (int t = 0; t < n; t++) *reinterpret_cast<u32x4 *>(out + t * P.fb + o) = *reinterpret_cast<const u32x4 *>(cur + t * P.fb + o);
                const u32x4 z = {0u, 0u, 0u, 0u};
                *reinterpret_cast<u32x4 *>(po_ + o) = z;
                *reinterpret_cast<u32x4 *>(so_ + 2 * o) = z;
                *reinterpret_cast<u32x4 *>(so_ + 2 * o + 16) = z;
            } else {
                for (int t = 0; t < n; t++)
                    for (int k = 0; k < nc; k++) out[t * P.fb + o + k] = cur[t * P.fb + o + k];
                for (int k = 0; k < nc; k++) { po_[o + k] = 0; so_[2 * (o + k)] = 0; so_[2 * (o + k) + 1] = 0; }
            }
        }
        return;
    }

    if (L.fast) {
        unsigned pr[DN_ROWS + 2][6], cr[DN_ROWS + 2][6]; // window rows y0 - 1 .. y0 + DN_ROWS (clamped) of the picture before / this one
        unsigned S[DN_ROWS][8];                          // two samples' states per register
        long long ro[DN_ROWS + 2];
#pragma unroll
        for (int rr = 0; rr < DN_ROWS + 2; rr++) ro[rr] = (long long)min(max(y0 - 1 + rr, 0), H - 1) * W;
        int t = 0;
        if (P.has_state) {
#pragma unroll
            for (int rr = 0; rr < DN_ROWS + 2; rr++) dn_load_row(pi_ + ro[rr], x0, W, pr[rr]);
#pragma unroll
            for (int r = 0; r < DN_ROWS; r++) {          // (rows past the plane: the last row's state, never stored)
                const u32x4 a = *reinterpret_cast<const u32x4 *>(si_ + 2 * (ro[r + 1] + x0));
                const u32x4 b = *reinterpret_cast<const u32x4 *>(si_ + 2 * (ro[r + 1] + x0) + 16);
                S[r][0] = a.x; S[r][1] = a.y; S[r][2] = a.z; S[r][3] = a.w;
                S[r][4] = b.x; S[r][5] = b.y; S[r][6] = b.z; S[r][7] = b.w;
            }
        } else {                                         // a stream's first picture: S' = 16 c, out = c
#pragma unroll
            for (int rr = 0; rr < DN_ROWS + 2; rr++) dn_load_row(cur + ro[rr], x0, W, pr[rr]);
#pragma unroll
            for (int r = 0; r < DN_ROWS; r++) {
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const unsigned w = pr[r + 1][1 + (j >> 1)] >> (16 * (j & 1));
                    S[r][j] = ((w & 0xffu) << 4) | ((w & 0xff00u) << 12);
                }
                if (y0 + r < H) {
                    u32x4 o;
                    o.x = pr[r + 1][1]; o.y = pr[r + 1][2]; o.z = pr[r + 1][3]; o.w = pr[r + 1][4];
                    *reinterpret_cast<u32x4 *>(out + ro[r + 1] + x0) = o;
                }
            }
            t = 1;
        }
        for (; t < n; t++) {
            const uint8_t *c = cur + t * P.fb;
#pragma unroll
            for (int rr = 0; rr < DN_ROWS + 2; rr++) dn_load_row(c + ro[rr], x0, W, cr[rr]);
            unsigned o[DN_ROWS][4];
#pragma unroll
            for (int r = 0; r < DN_ROWS; r++) o[r][0] = o[r][1] = o[r][2] = o[r][3] = 0u;
#pragma unroll
            for (int x = 0; x < 16; x++) {
                unsigned h[DN_ROWS + 2];                 // a window row's |cur - pin| sum
#pragma unroll
                for (int rr = 0; rr < DN_ROWS + 2; rr++) h[rr] = __builtin_amdgcn_sad_u8(dn_win(cr[rr], x), dn_win(pr[rr], x), 0u);
#pragma unroll
                for (int r = 0; r < DN_ROWS; r++) {
                    const int m0 = (int)(h[r] + h[r + 1] + h[r + 2]);
                    const int cv = (int)((cr[r + 1][1 + (x >> 2)] >> (8 * (x & 3))) & 0xffu);
                    const int sv = (int)((S[r][x >> 1] >> (16 * (x & 1))) & 0xffffu);
                    const unsigned s2 = (unsigned)dn_next(cv, sv, m0, ka, kb);
                    S[r][x >> 1] = (x & 1) ? (S[r][x >> 1] & 0xffffu) | (s2 << 16) : (S[r][x >> 1] & 0xffff0000u) | s2;
                    o[r][x >> 2] |= ((s2 + 8u) >> 4) << (8 * (x & 3));
                }
            }
#pragma unroll
            for (int r = 0; r < DN_ROWS; r++)
                if (y0 + r < H) {
                    u32x4 v;
                    v.x = o[r][0]; v.y = o[r][1]; v.z = o[r][2]; v.w = o[r][3];
                    *reinterpret_cast<u32x4 *>(out + t * P.fb + ro[r + 1] + x0) = v;
                }
#pragma unroll
            for (int rr = 0; rr < DN_ROWS + 2; rr++)
#pragma unroll
                for (int k = 0; k < 6; k++) pr[rr][k] = cr[rr][k];
        }
#pragma unroll
        for (int r = 0; r < DN_ROWS; r++)
            if (y0 + r < H) {
                u32x4 v, a, b;
                v.x = pr[r + 1][1]; v.y = pr[r + 1][2]; v.z = pr[r + 1][3]; v.w = pr[r + 1][4];
                a.x = S[r][0]; a.y = S[r][1]; a.z = S[r][2]; a.w = S[r][3];
                b.x = S[r][4]; b.y = S[r][5]; b.z = S[r][6]; b.w = S[r][7];
                *reinterpret_cast<u32x4 *>(po_ + ro[r + 1] + x0) = v;
                *reinterpret_cast<u32x4 *>(so_ + 2 * (ro[r + 1] + x0)) = a;
                *reinterpret_cast<u32x4 *>(so_ + 2 * (ro[r + 1] + x0) + 16) = b;
            }
        return;
    }

    // byte path: S lives in the output state between pictures (a sample's state is read and written by its own item only)
    for (int t = 0; t < n; t++) {
        const uint8_t *c = cur + t * P.fb;
        const uint8_t *p = t ? c - P.fb : (P.has_state ? pi_ : nullptr);
        const uint8_t *sp = t ? so_ : si_;
        for (int r = 0; r < DN_ROWS && y0 + r < H; r++) {
            const int y = y0 + r;
            for (int k = 0; k < nc; k++) {
                const int x = x0 + k;
                const long long i = (long long)y * W + x;
                const int cv = c[i];
                int s2 = 16 * cv;
                if (p) {
                    int m0 = 0;
                    for (int dy = -1; dy <= 1; dy++) {
                        const long long ry = (long long)min(max(y + dy, 0), H - 1) * W;
                        for (int dx = -1; dx <= 1; dx++) {
                            const long long j = ry + min(max(x + dx, 0), W - 1);
                            m0 += abs((int)c[j] - (int)p[j]);
                        }
                    }
                    s2 = dn_next(cv, (int)sp[2 * i] | ((int)sp[2 * i + 1] << 8), m0, ka, kb);
                }
                so_[2 * i] = (uint8_t)(s2 & 0xff);
                so_[2 * i + 1] = (uint8_t)(s2 >> 8);
                out[t * P.fb + i] = (uint8_t)((unsigned)(s2 + 8) >> 4);
            }
        }
    }
    {
        const uint8_t *c = cur + (long long)(n - 1) * P.fb;
        for (int r = 0; r < DN_ROWS && y0 + r < H; r++)
            for (int k = 0; k < nc; k++) {
                const long long i = (long long)(y0 + r) * W + x0 + k;
                po_[i] = c[i];
            }
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct dsvg_denoise {
    int device = 0, nsrc = 0;
    DnParams P;
    int nblocks = 0;
    size_t fb = 0;
    uint8_t *pin[2] = {nullptr, nullptr};// [nsrc] frames each: the state's pin, read from pin[flip] and written to pin[flip ^ 1]
    uint8_t *S = nullptr;                // [nsrc][2 * fb]: the state's S, updated in place (a sample's S is its own item's)
    int flip = 0;
    std::vector<unsigned char> valid;    // per source: the state holds a picture
    uint8_t *tmp = nullptr;              // _clip: the state a clip leaves (3 frames), allocated by the first call
};

extern "C" int dsv1_denoise_valid(const dsv1_denoise *dn);

extern "C" void dsvg_denoise_destroy(dsvg_denoise *d)
{
    if (!d) return;
    if (hipSetDevice(d->device) == hipSuccess) {
        for (int k = 0; k < 2; k++) if (d->pin[k]) (void)hipFree(d->pin[k]);
        if (d->S) (void)hipFree(d->S);
        if (d->tmp) (void)hipFree(d->tmp);
    }
    (void)hipGetLastError();
    delete d;
}

static int denoise_state(dsvg_denoise *d)
{
    HIPCHK(hipSetDevice(d->device));
    for (int k = 0; k < 2; k++) HIPCHK(hipMalloc((void **)&d->pin[k], d->fb * (size_t)d->nsrc + 256));
    HIPCHK(hipMalloc((void **)&d->S, 2 * d->fb * (size_t)d->nsrc + 256));
    return DSVG_OK;
}

extern "C" int dsvg_denoise_create(dsvg_denoise **out, int device, int w, int h, int subsamp, const dsv1_denoise *dn, int nsrc, int with_state)
{
    if (!out || w < 1 || h < 1 || nsrc < 1 || !dsv1_denoise_valid(dn)) { dsvg_set_error("bad noise filter arguments"); return DSVG_ERR_ARG; }
    *out = nullptr;
    if (dsvg_device_count() <= device || device < 0) { dsvg_set_error("HIP device %d not present", device); (void)hipGetLastError(); return DSVG_ERR_NODEVICE; }
    dsvg_denoise *d = new dsvg_denoise();
    d->device = device; d->nsrc = nsrc;
    d->valid.assign((size_t)nsrc, 0);
    const int cw = (w + (1 << ((subsamp >> 2) & 3)) - 1) >> ((subsamp >> 2) & 3), ch = (h + (1 << (subsamp & 3)) - 1) >> (subsamp & 3);
    memset(&d->P, 0, sizeof d->P);
    long long blocks = 0, off = 0;
    for (int k = 0; k < 3; k++) {
        DnPlane &L = d->P.pl[k];
        L.W = k ? cw : w; L.H = k ? ch : h;
        L.cpr = (L.W + 15) / 16;
        L.block0 = (int)blocks;
        L.off = off;
        L.T = k ? dn->chroma : dn->luma;
        if (L.T) {
            L.ka = (float)(12.0 / L.T);
            L.kb = (float)(4.0 - 12.0 + (L.T / 2 + 0.5) / L.T);
        }
        off += (long long)L.W * L.H;
        const long long runs = (L.H + DN_ROWS - 1) / DN_ROWS;
        blocks += (runs * L.cpr + DN_THREADS - 1) / DN_THREADS;
        // (the kernel's item index, block * DN_THREADS + thread, is an int)
        if (blocks > INT_MAX / DN_THREADS) { delete d; dsvg_set_error("frame too large for the noise filter's grid"); return DSVG_ERR_UNSUPPORTED; }
    }
    d->nblocks = (int)blocks;
    d->fb = (size_t)off;
    d->P.fb = off;
    const int rc = with_state ? denoise_state(d) : DSVG_OK;
    if (rc) { dsvg_denoise_destroy(d); return rc; }
    *out = d;
    return DSVG_OK;
}

// nsrc sources x n pictures ([source][picture]) -> the same; the state each source starts from (pin_in / s_in, null: none) and the
// one it leaves, each with its source-to-source distance
static int dn_launch(const dsvg_denoise *d, hipStream_t st, const uint8_t *src, int nsrc, int n, const uint8_t *pin_in, const uint8_t *s_in, size_t pin_in_stride,
                     size_t s_in_stride, uint8_t *pin_out, uint8_t *s_out, size_t pin_out_stride, size_t s_out_stride, uint8_t *dst)
{
    const size_t fb = d->fb;
    const bool has = pin_in && s_in;
    for (int s0 = 0; s0 < nsrc; s0 += 65535) {
        const int ns = std::min(65535, nsrc - s0);
        DnParams P = d->P;
        const uint8_t *s = src + (size_t)s0 * n * fb;
        uint8_t *o = dst + (size_t)s0 * n * fb;
        const uint8_t *pi = has ? pin_in + (size_t)s0 * pin_in_stride : nullptr, *si = has ? s_in + (size_t)s0 * s_in_stride : nullptr;
        uint8_t *po = pin_out + (size_t)s0 * pin_out_stride, *so = s_out + (size_t)s0 * s_out_stride;
        P.n = n; P.has_state = has;
        P.pin_in_stride = (long long)pin_in_stride; P.s_in_stride = (long long)s_in_stride;
        P.pin_out_stride = (long long)pin_out_stride; P.s_out_stride = (long long)s_out_stride;
        for (int k = 0; k < 3; k++) {
            const DnPlane &L = P.pl[k];
            uintptr_t m = (uintptr_t)s | (uintptr_t)o | (uintptr_t)fb | (uintptr_t)L.off | (uintptr_t)L.W | (uintptr_t)po | (uintptr_t)so |
                          (uintptr_t)pin_out_stride | (uintptr_t)s_out_stride;
            if (has) m |= (uintptr_t)pi | (uintptr_t)si | (uintptr_t)pin_in_stride | (uintptr_t)s_in_stride;
            P.pl[k].fast = !(m & 15);
        }
        hipLaunchKernelGGL(k_denoise, dim3(d->nblocks, ns), dim3(DN_THREADS), 0, st, P, s, o, pi, si, po, so);
    }
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}

// a session's call: n pictures of each of the nsrc sources; every source goes on from the state the call before left, and leaves its own
extern "C" int dsvg_denoise_run(dsvg_denoise *d, void *stream, const void *src_dev, int n, void *dst_dev)
{
    if (!d || !d->S || !src_dev || !dst_dev || n < 1) { dsvg_set_error("bad noise filter arguments"); return DSVG_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(d->device));
    const uint8_t *src = (const uint8_t *)src_dev;
    uint8_t *dst = (uint8_t *)dst_dev;
    const size_t fb = d->fb;
    const uint8_t *pi = d->pin[d->flip];
    uint8_t *po = d->pin[d->flip ^ 1];
    for (int s0 = 0; s0 < d->nsrc;) {                    // sources with and without a state: runs of either kind
        int s1 = s0 + 1;
        while (s1 < d->nsrc && d->valid[(size_t)s1] == d->valid[(size_t)s0]) s1++;
        const bool has = d->valid[(size_t)s0] != 0;
        const int rc = dn_launch(d, st, src + (size_t)s0 * n * fb, s1 - s0, n, has ? pi + (size_t)s0 * fb : nullptr, has ? d->S + (size_t)s0 * 2 * fb : nullptr, fb, 2 * fb,
                                 po + (size_t)s0 * fb, d->S + (size_t)s0 * 2 * fb, fb, 2 * fb, dst + (size_t)s0 * n * fb);
        if (rc) return rc;
        s0 = s1;
    }
    d->flip ^= 1;
    std::fill(d->valid.begin(), d->valid.end(), (unsigned char)1);
    return DSVG_OK;
}

// the standalone pass: n pictures of one stream from the state state_in (device, 3 frames' bytes, or nullptr: the stream starts here);
// state_out (device or nullptr) receives the state the clip leaves -- through a buffer of the filter's own, so it may be state_in
extern "C" int dsvg_denoise_clip(dsvg_denoise *d, void *stream, const void *src_dev, int n, const void *state_in_dev, void *state_out_dev, void *dst_dev)
{
    if (!d || !src_dev || !dst_dev || n < 1) { dsvg_set_error("bad noise filter arguments"); return DSVG_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(d->device));
    if (!d->tmp) HIPCHK(hipMalloc((void **)&d->tmp, 3 * d->fb + 256));
    const uint8_t *si = (const uint8_t *)state_in_dev;
    const int rc = dn_launch(d, st, (const uint8_t *)src_dev, 1, n, si, si ? si + d->fb : nullptr, 0, 0, d->tmp, d->tmp + d->fb, 0, 0, (uint8_t *)dst_dev);
    if (rc) return rc;
    if (state_out_dev) HIPCHK(hipMemcpyAsync(state_out_dev, d->tmp, 3 * d->fb, hipMemcpyDeviceToDevice, st));
    return DSVG_OK;
}

extern "C" int dsvg_denoise_reset(dsvg_denoise *d, int source)
{
    if (!d || source < -1 || source >= d->nsrc) return DSVG_ERR_ARG;
    for (int s = 0; s < d->nsrc; s++)
        if (source < 0 || s == source) d->valid[(size_t)s] = 0;
    return DSVG_OK;
}
