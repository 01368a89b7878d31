/* dsv1_deint.c -- deinterlacing (include/dsv1_api.h, Deinterlacing): validation, sizes and the standalone call.  The definition is
 * stated in numpy in tests/_deint.py; the kernel and its device plumbing: k_deint.hip; the sessions: dsv1_enc.c, dsv1_scale.c. */
#include "dsv1_host.h"

int dsv1_deint_valid(const dsv1_deint *di)
{
    return di && (di->mode == DSV1_DEINT_FRAME || di->mode == DSV1_DEINT_FIELD) && (di->tff == 0 || di->tff == 1);
}

int dsv1_deint_out_frames(const dsv1_deint *di, int n)
{
    if (!dsv1_deint_valid(di) || n < 0) return DSVG_ERR_ARG;
    if (di->mode == DSV1_DEINT_FIELD) return n > INT32_MAX / 2 ? DSVG_ERR_ARG : 2 * n;
    return n;
}

int dsv1_deinterlace_clip(int device, const void *src, int w, int h, int subsamp, int n, const void *prev, void *dst, const dsv1_deint *di,
                          int on_device)
{
    dsvg_deint *d = NULL;
    void *dsrc = NULL, *dprev = NULL, *ddst = NULL;
    size_t fb;
    int rc, nout, hs, vs;
    if (!src || !dst || n < 1 || device < 0 || w < 1 || h < 1) return DSVG_ERR_ARG;
    if (subsamp != DSV_SUBSAMP_444 && subsamp != DSV_SUBSAMP_422 && subsamp != DSV_SUBSAMP_420 && subsamp != DSV_SUBSAMP_411) return DSVG_ERR_ARG;
    if ((nout = dsv1_deint_out_frames(di, n)) < 0) return DSVG_ERR_ARG;
    hs = (subsamp >> 2) & 3; vs = subsamp & 3;
    fb = (size_t)w * h + 2 * (size_t)((w + (1 << hs) - 1) >> hs) * (size_t)((h + (1 << vs) - 1) >> vs);
    if ((rc = dsvg_deint_create(&d, device, w, h, subsamp, di, 1, 0))) return rc;
    if (on_device) rc = dsvg_deint_clip(d, src, n, prev, dst);
    else {
        rc = dsvg_deint_upload(d, 0, src, fb * (size_t)n, &dsrc);
        if (!rc && prev) rc = dsvg_deint_upload(d, 1, prev, fb, &dprev);
        if (!rc) rc = dsvg_deint_alloc(d, &ddst, fb * (size_t)nout);
        if (!rc) rc = dsvg_deint_clip(d, dsrc, n, dprev, ddst);
        if (!rc) rc = dsvg_deint_download(d, dst, ddst, fb * (size_t)nout);
    }
    if (!rc) rc = dsvg_deint_sync(d);
    dsvg_deint_destroy(d);                              /* (frees ddst: the deinterlacer owns what it allocated) */
    return rc;
}
