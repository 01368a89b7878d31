/* dsv1_orient.c -- the eight orientations (include/dsv1_api.h, Orientation): the host-only algebra of the codes and the standalone
 * call.  The definition is stated in numpy in tests/_orient.py; the kernels and their device plumbing: k_orient.hip; the sessions:
 * dsv1_srcchain.c, dsv1_enc.c, dsv1_scale.c.
 * A code is a bit set: bit 2 transposes first, bit 0 then mirrors the columns of the result, bit 1 its rows. */
#include "dsv1_host.h"

static int code_ok(int a) { return a >= 0 && a <= 7; }

int dsv1_orient_valid(int orient, int subsamp)
{
    if (!code_ok(orient)) return 0;
    if (subsamp != DSV_SUBSAMP_444 && subsamp != DSV_SUBSAMP_422 && subsamp != DSV_SUBSAMP_420 && subsamp != DSV_SUBSAMP_411) return 0;
    /* a transposed chroma plane is the output's chroma plane only where both shifts are equal */
    if ((orient & 4) && ((subsamp >> 2) & 3) != (subsamp & 3)) return 0;
    return 1;
}

int dsv1_orient_dims(int orient, int w, int h, int *ow, int *oh)
{
    if (!code_ok(orient) || w < 1 || h < 1 || !ow || !oh) return DSVG_ERR_ARG;
    *ow = orient & 4 ? h : w;
    *oh = orient & 4 ? w : h;
    return DSVG_OK;
}

/* a then b.  Moving b's transposition in front of a's mirrors exchanges them (mirroring columns and then transposing is transposing and
 * then mirroring rows); mirrors of one axis cancel in pairs. */
int dsv1_orient_compose(int a, int b)
{
    int fx, fy;
    if (!code_ok(a) || !code_ok(b)) return DSVG_ERR_ARG;
    fx = a & 1; fy = (a >> 1) & 1;
    if (b & 4) { const int t = fx; fx = fy; fy = t; }
    fx ^= b & 1; fy ^= (b >> 1) & 1;
    return ((a ^ b) & 4) | (fy << 1) | fx;
}

/* the mirrors undo themselves; behind a transposition they change places: only ROT90 and ROT270 are not their own inverses */
int dsv1_orient_inverse(int a)
{
    if (!code_ok(a)) return DSVG_ERR_ARG;
    return a == DSV1_ORIENT_ROT90 ? DSV1_ORIENT_ROT270 : a == DSV1_ORIENT_ROT270 ? DSV1_ORIENT_ROT90 : a;
}

int dsv1_orient_from_exif(int tag)
{
    static const int code[8] = {DSV1_ORIENT_NONE, DSV1_ORIENT_HFLIP, DSV1_ORIENT_ROT180, DSV1_ORIENT_VFLIP, DSV1_ORIENT_TRANSPOSE, DSV1_ORIENT_ROT90,
                                DSV1_ORIENT_TRANSVERSE, DSV1_ORIENT_ROT270};
    return tag >= 1 && tag <= 8 ? code[tag - 1] : DSVG_ERR_ARG;
}

/* the source sample at column p, row q is shown at column a p + c q, row b p + d q: with b = c = 0 columns stay columns and a sign is a
 * mirror; with a = d = 0 the display column is c q and the display row b p -- a transposition, then the mirrors the signs ask for */
int dsv1_orient_from_matrix(const int32_t m[9])
{
    const int32_t one = 65536;
    int32_t a, b, c, d;
    if (!m) return DSVG_ERR_ARG;
    a = m[0]; b = m[1]; c = m[3]; d = m[4];
    if (b == 0 && c == 0) {
        if ((a != one && a != -one) || (d != one && d != -one)) return DSVG_ERR_ARG;
        return (a < 0 ? 1 : 0) | (d < 0 ? 2 : 0);
    }
    if (a == 0 && d == 0) {
        if ((b != one && b != -one) || (c != one && c != -one)) return DSVG_ERR_ARG;
        return 4 | (c < 0 ? 1 : 0) | (b < 0 ? 2 : 0);
    }
    return DSVG_ERR_ARG;
}

int dsv1_orient_clip(int device, const void *src, int w, int h, int subsamp, int n, void *dst, int orient, int on_device)
{
    dsvg_orient *o = NULL;
    size_t bytes;
    int rc;
    if (!src || !dst || n < 1 || device < 0 || w < 1 || h < 1 || !dsv1_orient_valid(orient, subsamp)) return DSVG_ERR_ARG;
    bytes = dsv1_frame_bytes(w, h, subsamp) * (size_t)n;
    if ((rc = dsvg_orient_create(&o, device, orient, w, h, subsamp))) return rc;
    {
        const dsv1_clip_io io = {{src, NULL}, {bytes, 0}, {dst, NULL}, {bytes, 0}};
        rc = dsv1_pass_clip(device, DSV1_SRC_ORIENT, o, n, &io, on_device);
    }
    dsvg_orient_destroy(o);
    return rc;
}
