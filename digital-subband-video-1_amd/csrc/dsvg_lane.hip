// dsvg_lane.hip -- where a session's source-side work is enqueued (dsvg_pixfmt.h): one stream, one event, two upload buffers and the
// device memory handed out.  The passes (k_pixfmt.hip, k_rgb.hip, k_deint.hip, k_denoise.hip, k_scale.hip; the standalone export of
// k_pixout.hip) run on the lane's stream.
#include <algorithm>
#include <vector>
#include "dsvg_host.hpp"
#include "dsvg_pixfmt.h"

extern "C" int dsvg_ctx_load_wait(dsvg_ctx *ctx, void *event);

struct dsvg_lane {
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev = nullptr;
    uint8_t *up[2] = {nullptr, nullptr};
    size_t up_bytes[2] = {0, 0};
    std::vector<void *> owned;
};

extern "C" void dsvg_lane_destroy(dsvg_lane *l)
{
    if (!l) return;
    if (hipSetDevice(l->device) == hipSuccess) {
        if (l->st) (void)hipStreamSynchronize(l->st);
        for (void *p : l->owned) (void)hipFree(p);
        for (int k = 0; k < 2; k++) if (l->up[k]) (void)hipFree(l->up[k]);
        if (l->ev) (void)hipEventDestroy(l->ev);
        if (l->st) (void)hipStreamDestroy(l->st);
    }
    (void)hipGetLastError();
    delete l;
}

static int lane_device_side(dsvg_lane *l)
{
    HIPCHK(hipSetDevice(l->device));
    HIPCHK(hipStreamCreateWithFlags(&l->st, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&l->ev, hipEventDisableTiming));
    return DSVG_OK;
}

extern "C" int dsvg_lane_create(dsvg_lane **out, int device)
{
    if (!out) { dsvg_set_error("bad lane arguments"); return DSVG_ERR_ARG; }
    *out = nullptr;
    if (dsvg_device_count() <= device || device < 0) { dsvg_set_error("HIP device %d not present", device); (void)hipGetLastError(); return DSVG_ERR_NODEVICE; }
    dsvg_lane *l = new dsvg_lane();
    l->device = device;
    const int rc = lane_device_side(l);
    if (rc) { dsvg_lane_destroy(l); return rc; }
    *out = l;
    return DSVG_OK;
}

extern "C" int dsvg_lane_alloc(dsvg_lane *l, void **dptr, size_t bytes)
{
    if (!l || !dptr) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(l->device));
    const hipError_t e = hipMalloc(dptr, bytes + 256);
    if (e != hipSuccess) { (void)hipGetLastError(); *dptr = nullptr; dsvg_set_error("hipMalloc of %zu bytes failed", bytes); return DSVG_ERR_HIP; }
    l->owned.push_back(*dptr);
    return DSVG_OK;
}

// one allocation of dsvg_lane_alloc back (nullptr: nothing): whatever was enqueued may still read it, so the stream runs dry first
extern "C" int dsvg_lane_free(dsvg_lane *l, void *dptr)
{
    if (!l) return DSVG_ERR_ARG;
    if (!dptr) return DSVG_OK;
    const auto it = std::find(l->owned.begin(), l->owned.end(), dptr);
    if (it == l->owned.end()) { dsvg_set_error("not an allocation of this lane"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(l->device));
    HIPCHK(hipStreamSynchronize(l->st));
    l->owned.erase(it);
    HIPCHK(hipFree(dptr));
    return DSVG_OK;
}

// bytes -> upload buffer `buf` (0 / 1) on the lane's stream: behind the pass that read the buffer last
static int lane_copy(dsvg_lane *l, int buf, const void *from, size_t bytes, void **dptr, hipMemcpyKind kind)
{
    if (!l || !from || !dptr || !bytes || buf < 0 || buf > 1) { dsvg_set_error("bad lane upload arguments"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(l->device));
    if (l->up_bytes[buf] < bytes) {
        if (l->up[buf]) { HIPCHK(hipStreamSynchronize(l->st)); HIPCHK(hipFree(l->up[buf])); l->up[buf] = nullptr; l->up_bytes[buf] = 0; }
        HIPCHK(hipMalloc((void **)&l->up[buf], bytes + 256));
        l->up_bytes[buf] = bytes;
    }
    HIPCHK(hipMemcpyAsync(l->up[buf], from, bytes, kind, l->st));
    *dptr = l->up[buf];
    return DSVG_OK;
}
extern "C" int dsvg_lane_upload(dsvg_lane *l, int buf, const void *host, size_t bytes, void **dptr)
{
    return lane_copy(l, buf, host, bytes, dptr, hipMemcpyHostToDevice);
}
// the same from device memory (a copy the caller's clip need not outlive)
extern "C" int dsvg_lane_copy_in(dsvg_lane *l, int buf, const void *dev, size_t bytes, void **dptr)
{
    return lane_copy(l, buf, dev, bytes, dptr, hipMemcpyDeviceToDevice);
}

// device memory to device memory on the lane's stream, neither side an upload buffer (a pass that works in place on a copy)
extern "C" int dsvg_lane_copy_dd(dsvg_lane *l, void *dst_dev, const void *src_dev, size_t bytes)
{
    if (!l || !dst_dev || !src_dev || !bytes) { dsvg_set_error("bad lane copy arguments"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(l->device));
    HIPCHK(hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, l->st));
    return DSVG_OK;
}

extern "C" int dsvg_lane_download(dsvg_lane *l, void *host, const void *dptr, size_t bytes)
{
    if (!l || !host || !dptr) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(l->device));
    HIPCHK(hipMemcpyAsync(host, dptr, bytes, hipMemcpyDeviceToHost, l->st));
    HIPCHK(hipStreamSynchronize(l->st));
    return DSVG_OK;
}

extern "C" int dsvg_lane_order(dsvg_lane *l, dsvg_ctx *ctx)
{
    if (!l || !ctx) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(l->device));
    HIPCHK(hipEventRecord(l->ev, l->st));
    return dsvg_ctx_load_wait(ctx, (void *)l->ev);
}

extern "C" int dsvg_lane_sync(dsvg_lane *l)
{
    if (!l) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(l->device));
    HIPCHK(hipStreamSynchronize(l->st));
    return DSVG_OK;
}

extern "C" void *dsvg_lane_stream(dsvg_lane *l) { return l ? (void *)l->st : nullptr; }
