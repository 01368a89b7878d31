// k_overlay.hip -- the overlay pass (include/dsv1_api.h, Overlays; the plan: dsvg_overlay_plan.h; stated in numpy in
// tests/_overlay.py): a list of timed bitmaps alpha-blended IN PLACE onto a clip of tightly packed planar 8-bit frames.
//
// The bitmaps go into device memory once, at create: per overlay Y, U, V, A and the chroma alpha A_c (built on the host).  A call is
// planned on the host (dsvg_overlay_plan): the items (overlay, source, frame, op) with op > 0, each with a layer.  Every item gives
// three ENTRIES, one per plane: a rectangle of pw x ph bytes somewhere in the clip, the bitmap plane and the alpha plane that go with
// it, and op.  The entries of a layer lie together in the table and never touch the same byte, so a layer is ONE launch; layer k + 1
// reads what layer k wrote, so the layers are launched one after the other on the stream.
//
// k_overlay: a unit is one 16-byte ALIGNED chunk of one row of an entry's rectangle (a row starts at any byte address: x is aligned
// to the subsampling only and the plane's width may be odd; cpr = (pw + 30) / 16 units cover any row).  A block is 256 units of ONE
// entry -- a tile -- and the grid is the sum of the entries' tiles: the cost is the overlays' area, not the picture's.  A block finds
// its entry by bisection over the tiles' prefix sums (uniform over the block).  A whole chunk is one aligned 16-byte load of the
// clip, one unaligned 16-byte load each of the bitmap and the alpha (which name exactly the 16 samples, so nothing outside the
// planes is read), 16 blends and one aligned 16-byte store.  A partial chunk -- a row's head and tail -- moves its bytes one by one:
// no byte outside the rectangle is written, not even with the value it held, because a neighbouring entry of the same layer may be
// writing it.
//   k = alpha * op;  out = (in * (65280 - k) + ov * k + 32640) / 65280  =  ((...) >> 8) / 255, the numerator below 2^24.
#include <algorithm>
#include <climits>
#include "dsvg_host.hpp"
#include "dsvg_pixfmt.h"
#include "dsvg_overlay_plan.h"

#define OV_THREADS 256

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4a1 __attribute__((ext_vector_type(4), aligned(1)));       // 16 bytes at any address

struct OvEntry {
    int tile0;                           // first tile of the entry among its layer's
    int pw, ph, cpr;                     // the rectangle in this plane; chunks per row
    int dpitch, op;                      // the clip plane's width; the picture's opacity, 1 .. 256
    long long doff;                      // the rectangle's top left in the clip
    long long boff, aoff;                // the bitmap's plane and its alpha plane in the packed bitmaps (pitch pw)
};

static __device__ __forceinline__ unsigned ov_blend(unsigned in, unsigned ov, unsigned alpha, unsigned op)
{
    const unsigned k = alpha * op;
    return ((in * (65280u - k) + ov * k + 32640u) >> 8) / 255u;
}

static __device__ __forceinline__ unsigned ov_blend4(unsigned in, unsigned ov, unsigned alpha, unsigned op)
{
    unsigned r = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) r |= ov_blend((in >> (8 * b)) & 0xffu, (ov >> (8 * b)) & 0xffu, (alpha >> (8 * b)) & 0xffu, op) << (8 * b);
    return r;
}

__global__ __launch_bounds__(OV_THREADS) void k_overlay(const OvEntry *__restrict__ ent, int nent, const uint8_t *__restrict__ bmp, uint8_t *clip)
{
    const int tile = (int)blockIdx.x;
    int lo = 0, hi = nent - 1;
    while (lo < hi) {                    // the last entry whose first tile is not behind this one
        const int mid = (lo + hi + 1) >> 1;
        if (ent[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
    }
    const OvEntry E = ent[lo];
    const int unit = (tile - E.tile0) * OV_THREADS + (int)threadIdx.x;
    const int Y = unit / E.cpr;
    if (Y >= E.ph) return;
    uint8_t *row = clip + E.doff + (long long)Y * E.dpitch;
    const int x0 = 16 * (unit - Y * E.cpr) - (int)((uintptr_t)row & 15);
    if (x0 >= E.pw) return;
    const uint8_t *orow = bmp + E.boff + (long long)Y * E.pw;
    const uint8_t *arow = bmp + E.aoff + (long long)Y * E.pw;
    const unsigned op = (unsigned)E.op;
    if (x0 >= 0 && x0 + 16 <= E.pw) {
        const u32x4 d = *reinterpret_cast<const u32x4 *>(row + x0);
        const u32x4a1 o = *reinterpret_cast<const u32x4a1 *>(orow + x0);
        const u32x4a1 a = *reinterpret_cast<const u32x4a1 *>(arow + x0);
        *reinterpret_cast<u32x4 *>(row + x0) = u32x4{ov_blend4(d.x, o.x, a.x, op), ov_blend4(d.y, o.y, a.y, op), ov_blend4(d.z, o.z, a.z, op),
                                                     ov_blend4(d.w, o.w, a.w, op)};
    } else {
        for (int b = 0; b < 16; b++) {
            const int x = x0 + b;
            if (x >= 0 && x < E.pw) row[x] = (uint8_t)ov_blend(row[x], orow[x], arow[x], op);
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct OvBitmap { long long off[5]; };  // Y, U, V, A, A_c in the packed bitmaps

struct dsvg_overlay {
    int device = 0, w = 0, h = 0, subsamp = 0, nsrc = 0;
    std::vector<dsv1_overlay> list;      // the placements (planes: not kept)
    std::vector<OvBitmap> bmp;
    uint8_t *bmp_dev = nullptr;
    std::vector<dsv1_overlay_item> items;
    OvEntry *tab_host[2] = {nullptr, nullptr};          // pinned, per call parity
    OvEntry *tab_dev[2] = {nullptr, nullptr};
    size_t tab_room[2] = {0, 0};
};

extern "C" void dsvg_overlay_destroy(dsvg_overlay *o)
{
    if (!o) return;
    if (hipSetDevice(o->device) == hipSuccess) {
        if (o->bmp_dev) (void)hipFree(o->bmp_dev);
        for (int k = 0; k < 2; k++) {
            if (o->tab_dev[k]) (void)hipFree(o->tab_dev[k]);
            if (o->tab_host[k]) (void)hipHostFree(o->tab_host[k]);
        }
    }
    (void)hipGetLastError();
    delete o;
}

// A_c[Y][X] = r(sum / count) over the alpha samples the chroma sample covers
static void ov_chroma_alpha(const uint8_t *A, int w, int h, int hs, int vs, uint8_t *Ac)
{
    const int cw = rsu(w, hs), ch = rsu(h, vs);
    for (int Y = 0; Y < ch; Y++)
        for (int X = 0; X < cw; X++) {
            const int x1 = std::min(w, (X + 1) << hs), y1 = std::min(h, (Y + 1) << vs);
            int sum = 0, cnt = 0;
            for (int y = Y << vs; y < y1; y++)
                for (int x = X << hs; x < x1; x++) { sum += A[(size_t)y * w + x]; cnt++; }
            Ac[(size_t)Y * cw + X] = (uint8_t)((2 * sum + cnt) / (2 * cnt));
        }
}

static int ov_device_side(dsvg_overlay *o, const dsv1_overlay *list, int n)
{
    const int hs = fmt_hs(o->subsamp), vs = fmt_vs(o->subsamp);
    long long total = 0;
    for (int i = 0; i < n; i++) {
        const long long yb = (long long)list[i].w * list[i].h, cb = (long long)rsu(list[i].w, hs) * rsu(list[i].h, vs);
        OvBitmap B;
        B.off[0] = total; B.off[1] = total + yb; B.off[2] = total + yb + cb; B.off[3] = total + yb + 2 * cb; B.off[4] = total + 2 * yb + 2 * cb;
        total += 2 * yb + 3 * cb;
        o->bmp.push_back(B);
    }
    std::vector<uint8_t> host((size_t)total);
    for (int i = 0; i < n; i++) {
        const OvBitmap &B = o->bmp[i];
        memcpy(&host[(size_t)B.off[0]], list[i].planes, (size_t)(B.off[4] - B.off[0]));
        ov_chroma_alpha(&host[(size_t)B.off[3]], list[i].w, list[i].h, hs, vs, &host[(size_t)B.off[4]]);
    }
    HIPCHK(hipSetDevice(o->device));
    HIPCHK(hipMalloc((void **)&o->bmp_dev, (size_t)total + 256));
    HIPCHK(hipMemcpy(o->bmp_dev, host.data(), (size_t)total, hipMemcpyHostToDevice));
    return DSVG_OK;
}

extern "C" int dsvg_overlay_create(dsvg_overlay **out, int device, const dsv1_overlay *list, int n, int w, int h, int subsamp, int nsrc)
{
    if (!out || !list || n < 1 || n > DSV1_MAX_OVERLAYS) { dsvg_set_error("bad overlay arguments"); return DSVG_ERR_ARG; }
    *out = nullptr;
    for (int i = 0; i < n; i++)
        if (!dsvg_overlay_valid(&list[i], w, h, subsamp, nsrc)) { dsvg_set_error("overlay %d is not valid on %dx%d, subsampling 0x%x, %d sources", i, w, h, subsamp, nsrc); return DSVG_ERR_ARG; }
    if (dsvg_device_count() <= device || device < 0) { dsvg_set_error("HIP device %d not present", device); (void)hipGetLastError(); return DSVG_ERR_NODEVICE; }
    dsvg_overlay *o = new dsvg_overlay();
    o->device = device; o->w = w; o->h = h; o->subsamp = subsamp; o->nsrc = nsrc;
    o->list.assign(list, list + n);
    const int rc = ov_device_side(o, list, n);
    for (auto &p : o->list) p.planes = nullptr;         // (the caller's memory is free on return)
    if (rc) { dsvg_overlay_destroy(o); return rc; }
    *out = o;
    return DSVG_OK;
}

// the items a call of nframes frames per source would blend (nothing is kept, nothing touches the device)
extern "C" long long dsvg_overlay_active(const dsvg_overlay *o, int nframes, const int64_t *counters)
{
    if (!o || !counters || nframes < 1) return 0;
    return dsvg_overlay_plan(o->list.data(), (int)o->list.size(), o->nsrc, nframes, counters, nullptr, 0, nullptr);
}

static int ov_table_room(dsvg_overlay *o, hipStream_t st, int par, size_t n)
{
    if (o->tab_room[par] >= n) return DSVG_OK;
    HIPCHK(hipStreamSynchronize(st));                   // (the last call of this parity may still read its table)
    if (o->tab_dev[par]) { HIPCHK(hipFree(o->tab_dev[par])); o->tab_dev[par] = nullptr; }
    if (o->tab_host[par]) { HIPCHK(hipHostFree(o->tab_host[par])); o->tab_host[par] = nullptr; }
    o->tab_room[par] = 0;
    const size_t room = std::max<size_t>(n + n / 2, 96);
    HIPCHK(hipHostMalloc((void **)&o->tab_host[par], room * sizeof(OvEntry), hipHostMallocDefault));
    HIPCHK(hipMalloc((void **)&o->tab_dev[par], room * sizeof(OvEntry)));
    o->tab_room[par] = room;
    return DSVG_OK;
}

// clip_dev: [source][nframes] frames of the overlay's geometry, blended in place; counters[s]: the picture source s's first frame is.
// The call's table goes up on the stream into the buffer of parity `par` (a call of that parity must have run before the next one of
// the same parity is enqueued from another thread of control: a session collects it first).  Nothing active: nothing enqueued.
extern "C" int dsvg_overlay_run(dsvg_overlay *o, void *stream, int par, void *clip_dev, int nframes, const int64_t *counters)
{
    if (!o || !clip_dev || !counters || nframes < 1 || par < 0 || par > 1) { dsvg_set_error("bad overlay arguments"); return DSVG_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    const int hs = fmt_hs(o->subsamp), vs = fmt_vs(o->subsamp), n = (int)o->list.size();
    const long long cnt = dsvg_overlay_plan(o->list.data(), n, o->nsrc, nframes, counters, nullptr, 0, nullptr);
    if (!cnt) return DSVG_OK;
    if (cnt > INT_MAX / 8) { dsvg_set_error("too many overlay items in one call"); return DSVG_ERR_UNSUPPORTED; }
    int nlayers = 0;
    o->items.resize((size_t)cnt);
    (void)dsvg_overlay_plan(o->list.data(), n, o->nsrc, nframes, counters, o->items.data(), cnt, &nlayers);
    HIPCHK(hipSetDevice(o->device));
    int rc = ov_table_room(o, st, par, (size_t)cnt * 3);
    if (rc) return rc;
    // the entries, layer by layer (a counting sort: the order inside a layer does not matter, its entries are disjoint)
    std::vector<int> first(nlayers + 2, 0), ntiles(nlayers + 1, 0);
    for (const auto &it : o->items) first[it.layer + 1] += 3;
    for (int l = 1; l <= nlayers + 1; l++) first[l] += first[l - 1];
    std::vector<int> at(first.begin(), first.end() - 1);         // at[l]: where layer l's next entry goes
    const int cw = rsu(o->w, hs), chh = rsu(o->h, vs);
    const long long fb = (long long)o->w * o->h + 2ll * cw * chh;
    OvEntry *tab = o->tab_host[par];
    for (const auto &it : o->items) {
        const dsv1_overlay &p = o->list[it.overlay];
        const OvBitmap &B = o->bmp[it.overlay];
        const long long frame = ((long long)it.source * nframes + it.frame) * fb;
        for (int k = 0; k < 3; k++) {
            OvEntry &E = tab[at[it.layer]++];
            const int PW = k ? cw : o->w;
            E.pw = k ? rsu(p.w, hs) : p.w; E.ph = k ? rsu(p.h, vs) : p.h;
            E.cpr = (E.pw + 30) / 16;
            E.dpitch = PW; E.op = it.op;
            E.doff = frame + (k == 0 ? 0 : (long long)o->w * o->h + (k - 1) * (long long)cw * chh) + (long long)(k ? p.y >> vs : p.y) * PW + (k ? p.x >> hs : p.x);
            E.boff = B.off[k]; E.aoff = B.off[k ? 4 : 3];
            E.tile0 = 0;
        }
    }
    for (int l = 1; l <= nlayers; l++) {
        long long t = 0;
        for (int e = first[l]; e < first[l + 1]; e++) {
            tab[e].tile0 = (int)t;
            t += ((long long)tab[e].ph * tab[e].cpr + OV_THREADS - 1) / OV_THREADS;
            // (the kernel's unit index, tile * OV_THREADS + thread, is an int)
            if (t > INT_MAX / OV_THREADS) { dsvg_set_error("overlay area too large for one launch"); return DSVG_ERR_UNSUPPORTED; }
        }
        ntiles[l] = (int)t;
    }
    HIPCHK(hipMemcpyAsync(o->tab_dev[par], tab, (size_t)cnt * 3 * sizeof(OvEntry), hipMemcpyHostToDevice, st));
    for (int l = 1; l <= nlayers; l++)
        hipLaunchKernelGGL(k_overlay, dim3(ntiles[l]), dim3(OV_THREADS), 0, st, o->tab_dev[par] + first[l], first[l + 1] - first[l],
                           (const uint8_t *)o->bmp_dev, (uint8_t *)clip_dev);
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}
