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
    size_t fb;
    int rc, nout;
    if (!src || !dst || n < 1 || device < 0 || w < 1 || h < 1) return DSVG_ERR_ARG;
    if (subsamp != DSV_SUBSAMP_444 && subsamp != DSV_SUBSAMP_422 && subsamp != DSV_SUBSAMP_420 && subsamp != DSV_SUBSAMP_411) return DSVG_ERR_ARG;
    if ((nout = dsv1_deint_out_frames(di, n)) < 0) return DSVG_ERR_ARG;
    fb = dsv1_frame_bytes(w, h, subsamp);
    if ((rc = dsvg_deint_create(&d, device, w, h, subsamp, di, 1, 0))) return rc;
    {
        const dsv1_clip_io io = {{src, prev}, {fb * (size_t)n, fb}, {dst, NULL}, {fb * (size_t)nout, 0}};
        rc = dsv1_pass_clip(device, DSV1_SRC_DEINTERLACE, d, n, &io, on_device);
    }
    dsvg_deint_destroy(d);
    return rc;
}
