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

size_t dsv1_denoise_state_bytes(int w, int h, int subsamp)
{
    if (w < 1 || h < 1 || !subsamp_known(subsamp)) return 0;
    return 3 * dsv1_frame_bytes(w, h, subsamp);
}

int dsv1_denoise_clip(int device, const void *src, int w, int h, int subsamp, int n, const void *state_in, void *state_out, void *dst,
                      const dsv1_denoise *dn, int on_device)
{
    dsvg_denoise *d = NULL;
    size_t fb;
    int rc;
    if (!src || !dst || n < 1 || device < 0 || w < 1 || h < 1 || !subsamp_known(subsamp) || !dsv1_denoise_valid(dn)) return DSVG_ERR_ARG;
    fb = dsv1_frame_bytes(w, h, subsamp);
    if ((rc = dsvg_denoise_create(&d, device, w, h, subsamp, dn, 1, 0))) return rc;
    {
        const dsv1_clip_io io = {{src, state_in}, {fb * (size_t)n, 3 * fb}, {dst, state_out}, {fb * (size_t)n, 3 * fb}};
        rc = dsv1_pass_clip(device, DSV1_SRC_DENOISE, d, n, &io, on_device);
    }
    dsvg_denoise_destroy(d);
    return rc;
}
