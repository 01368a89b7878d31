/* dsv1_ivtc.c -- inverse telecine and field order detection (include/dsv1_api.h, Inverse telecine): validation, sizes, the host side
 * of the decision rules (../dsvg_ivtc_rules.h, which the kernels compile too), the vote and the standalone calls.  The definition is
 * stated in numpy in tests/_ivtc.py; the kernels and their device plumbing: k_ivtc.hip; the sessions: dsv1_srcchain.c, dsv1_enc.c,
 * dsv1_scale.c. */
#include "dsv1_host.h"
#include "../dsvg_ivtc_rules.h"

/* the sums are uint32: 255 * w * h stays below UINT32_MAX, which marks a first picture's D */
#define IVTC_MAX_LUMA 16843008

static int subsamp_known(int subsamp)
{
    return subsamp == DSV_SUBSAMP_444 || subsamp == DSV_SUBSAMP_422 || subsamp == DSV_SUBSAMP_420 || subsamp == DSV_SUBSAMP_411;
}

static int geom_known(int w, int h, int subsamp)
{
    return w >= 1 && h >= 1 && (int64_t)w * h <= IVTC_MAX_LUMA && subsamp_known(subsamp);
}

int dsv1_ivtc_valid(const dsv1_ivtc *iv)
{
    return iv && (iv->tff == 0 || iv->tff == 1) && iv->nt >= 0 && iv->nt <= 254 && !iv->reserved[0] && !iv->reserved[1];
}

int dsv1_ivtc_out_frames(const dsv1_ivtc *iv, int n)
{
    if (!dsv1_ivtc_valid(iv) || n < 0 || n % IVTC_CYCLE) return DSVG_ERR_ARG;
    return n / IVTC_CYCLE * 4;
}

size_t dsv1_ivtc_state_bytes(int w, int h, int subsamp)
{
    if (w < 1 || h < 1 || !subsamp_known(subsamp)) return 0;
    return dsv1_frame_bytes(w, h, subsamp) + (size_t)w * (size_t)h;
}

int dsv1_ivtc_match(const uint32_t *metrics, int n, int first_has_prev, int tff, uint8_t *match)
{
    int t;
    if (!metrics || !match || n < 0 || (tff != 0 && tff != 1)) return DSVG_ERR_ARG;
    for (t = 0; t < n; t++) match[t] = (uint8_t)ivtc_match_rule(metrics + 4 * (size_t)t, t > 0 || first_has_prev, tff ? 0 : 1);
    return DSVG_OK;
}

int dsv1_ivtc_pick(const uint32_t *D, int n, uint8_t *drop)
{
    int c;
    if (!D || !drop || n < 0 || n % IVTC_CYCLE) return DSVG_ERR_ARG;
    for (c = 0; c < n / IVTC_CYCLE; c++) drop[c] = (uint8_t)ivtc_pick_rule(D + IVTC_CYCLE * (size_t)c);
    return DSVG_OK;
}

int dsv1_field_order_from_metrics(const uint32_t *metrics, int n, int first_has_prev)
{
    int64_t tv = 0, bv = 0;
    int t;
    if (!metrics || n < 1) return DSVG_ERR_ARG;
    for (t = first_has_prev ? 0 : 1; t < n; t++) {
        const uint32_t *m = metrics + 4 * (size_t)t;
        if (m[2] < m[3]) tv++;
        else if (m[3] < m[2]) bv++;
    }
    return tv > 2 * bv ? 1 : bv > 2 * tv ? 0 : -1;
}

int dsv1_field_metrics_clip(int device, const void *src, int w, int h, int subsamp, int n, const void *prev, int nt, uint32_t *metrics, int on_device)
{
    dsvg_lane *l = NULL;
    void *d, *dm = NULL;
    size_t fb, mb;
    int rc;
    if (!src || !metrics || n < 1 || device < 0 || nt < 0 || nt > 254 || !geom_known(w, h, subsamp)) return DSVG_ERR_ARG;
    if ((size_t)n > SIZE_MAX / (4 * sizeof(uint32_t))) return DSVG_ERR_ARG;
    fb = dsv1_frame_bytes(w, h, subsamp);
    mb = 4 * sizeof(uint32_t) * (size_t)n;
    if ((rc = dsvg_lane_create(&l, device))) return rc;
    if (!on_device) {
        if (!(rc = dsvg_lane_upload(l, 0, src, fb * (size_t)n, &d))) src = d;
        if (!rc && prev && !(rc = dsvg_lane_upload(l, 1, prev, fb, &d))) prev = d;
    }
    if (!rc) rc = dsvg_lane_alloc(l, &dm, mb);
    if (!rc) rc = dsvg_field_metrics_run(device, dsvg_lane_stream(l), src, w, h, subsamp, n, prev, nt, dm);
    if (!rc) rc = dsvg_lane_download(l, metrics, dm, mb);
    if (!rc) rc = dsvg_lane_sync(l);
    dsvg_lane_destroy(l);                               /* (waits for the stream; frees what the call allocated) */
    return rc;
}

int dsv1_detect_field_order_clip(int device, const void *src, int w, int h, int subsamp, int n, int nt, int on_device)
{
    uint32_t *m;
    int rc;
    if (!src || n < 1 || device < 0 || nt < 0 || nt > 254 || !geom_known(w, h, subsamp)) return DSVG_ERR_ARG;
    if ((size_t)n > SIZE_MAX / (4 * sizeof(uint32_t))) return DSVG_ERR_ARG;
    m = (uint32_t *)malloc(4 * sizeof(uint32_t) * (size_t)n);
    if (!m) return DSVG_ERR_NOMEM;
    rc = dsv1_field_metrics_clip(device, src, w, h, subsamp, n, NULL, nt, m, on_device);
    if (!rc) rc = dsv1_field_order_from_metrics(m, n, 0);
    else if (rc == DSVG_ERR_HIP) rc = DSVG_ERR_NODEVICE;       /* (-1 is an answer) */
    free(m);
    return rc;
}

int dsv1_ivtc_clip(int device, const void *src, int w, int h, int subsamp, int n, const void *state_in, void *state_out, void *dst,
                   const dsv1_ivtc *iv, uint8_t *match_out, uint8_t *drop_out, int on_device)
{
    dsvg_ivtc *p = NULL;
    dsvg_lane *l = NULL;
    const void *dm, *dd;
    void *d, *ddst = dst, *dso = state_out;
    size_t fb, sb;
    int rc, nout;
    if (!src || !dst || n < IVTC_CYCLE || device < 0 || !geom_known(w, h, subsamp)) return DSVG_ERR_ARG;
    if ((nout = dsv1_ivtc_out_frames(iv, n)) < 0) return DSVG_ERR_ARG;
    fb = dsv1_frame_bytes(w, h, subsamp);
    sb = dsv1_ivtc_state_bytes(w, h, subsamp);
    if ((rc = dsvg_ivtc_create(&p, device, w, h, subsamp, iv, 1, n, 0))) return rc;
    if (!(rc = dsvg_lane_create(&l, device))) {
        if (!on_device) {
            if (!(rc = dsvg_lane_upload(l, 0, src, fb * (size_t)n, &d))) src = d;
            if (!rc && state_in && !(rc = dsvg_lane_upload(l, 1, state_in, sb, &d))) state_in = d;
            if (!rc) rc = dsvg_lane_alloc(l, &ddst, fb * (size_t)nout);
            if (!rc && state_out) rc = dsvg_lane_alloc(l, &dso, sb);
        }
        if (!rc) rc = dsvg_ivtc_clip(p, dsvg_lane_stream(l), src, state_in, dso, ddst);
        if (!rc && !on_device) rc = dsvg_lane_download(l, dst, ddst, fb * (size_t)nout);
        if (!rc && !on_device && state_out) rc = dsvg_lane_download(l, state_out, dso, sb);
        dsvg_ivtc_tables(p, &dm, &dd);
        if (!rc && match_out) rc = dsvg_lane_download(l, match_out, dm, (size_t)n);
        if (!rc && drop_out) rc = dsvg_lane_download(l, drop_out, dd, (size_t)(n / IVTC_CYCLE));
        if (!rc) rc = dsvg_lane_sync(l);
        dsvg_lane_destroy(l);                           /* (waits for the stream; frees what the call allocated) */
    }
    dsvg_ivtc_destroy(p);
    return rc;
}
