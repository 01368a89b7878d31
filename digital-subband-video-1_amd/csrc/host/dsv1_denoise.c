/* dsv1_denoise.c -- temporal noise reduction (include/dsv1_api.h, Temporal noise reduction): validation, sizes and the standalone call.
 * The definition is stated in numpy in tests/_denoise.py; the kernel and its device plumbing: k_denoise.hip; the sessions: dsv1_enc.c,
 * dsv1_scale.c. */
#include "dsv1_host.h"

int dsv1_denoise_valid(const dsv1_denoise *dn)
{
    return dn && dn->luma >= 0 && dn->luma <= DSV1_DENOISE_MAX && dn->chroma >= 0 && dn->chroma <= DSV1_DENOISE_MAX && (dn->luma || dn->chroma);
}

static int subsamp_known(int subsamp)
{
    return subsamp == DSV_SUBSAMP_444 || subsamp == DSV_SUBSAMP_422 || subsamp == DSV_SUBSAMP_420 || subsamp == DSV_SUBSAMP_411;
}

static size_t frame_bytes(int w, int h, int subsamp)
{
    const int hs = (subsamp >> 2) & 3, vs = subsamp & 3;
    return (size_t)w * h + 2 * (size_t)((w + (1 << hs) - 1) >> hs) * (size_t)((h + (1 << vs) - 1) >> vs);
}

size_t dsv1_denoise_state_bytes(int w, int h, int subsamp)
{
    if (w < 1 || h < 1 || !subsamp_known(subsamp)) return 0;
    return 3 * frame_bytes(w, h, subsamp);
}

int dsv1_denoise_clip(int device, const void *src, int w, int h, int subsamp, int n, const void *state_in, void *state_out, void *dst,
                      const dsv1_denoise *dn, int on_device)
{
    dsvg_denoise *d = NULL;
    void *dsrc = NULL, *dsin = NULL, *dsout = NULL, *ddst = NULL;
    size_t fb;
    int rc;
    if (!src || !dst || n < 1 || device < 0 || w < 1 || h < 1 || !subsamp_known(subsamp) || !dsv1_denoise_valid(dn)) return DSVG_ERR_ARG;
    fb = frame_bytes(w, h, subsamp);
    if ((rc = dsvg_denoise_create(&d, device, w, h, subsamp, dn, 1, 0))) return rc;
    if (on_device) rc = dsvg_denoise_clip(d, src, n, state_in, state_out, dst);
    else {
        rc = dsvg_denoise_upload(d, 0, src, fb * (size_t)n, &dsrc);
        if (!rc && state_in) rc = dsvg_denoise_upload(d, 1, state_in, 3 * fb, &dsin);
        if (!rc) rc = dsvg_denoise_alloc(d, &ddst, fb * (size_t)n);
        if (!rc && state_out) rc = dsvg_denoise_alloc(d, &dsout, 3 * fb);
        if (!rc) rc = dsvg_denoise_clip(d, dsrc, n, dsin, dsout, ddst);
        if (!rc) rc = dsvg_denoise_download(d, dst, ddst, fb * (size_t)n);
        if (!rc && state_out) rc = dsvg_denoise_download(d, state_out, dsout, 3 * fb);
    }
    if (!rc) rc = dsvg_denoise_sync(d);
    dsvg_denoise_destroy(d);                            /* (frees what the filter allocated) */
    return rc;
}
