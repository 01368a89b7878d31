/* dsvg_ivtc_rules.h -- the two decision rules of the inverse telecine (include/dsv1_api.h, Inverse telecine; stated in numpy in
 * tests/_ivtc.py), shared between the host (host/dsv1_ivtc.c: dsv1_ivtc_match, dsv1_ivtc_pick) and the device (k_ivtc.hip:
 * k_ivtc_match, k_ivtc_pick), so that what the CPU suite tests through the C ABI is what the kernels run. */
#ifndef DSVG_IVTC_RULES_H
#define DSVG_IVTC_RULES_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IVTC_HD __host__ __device__ static inline
#else
#define IVTC_HD static inline
#endif

#define IVTC_MATCH_C 0          /* the other field is the frame's own */
#define IVTC_MATCH_P 1          /* the other field is the frame before's */
#define IVTC_CYCLE 5

/* m: mc0 mc1 mp0 mp1 of one frame; p: the parity of the first field in time.  P only where it is strictly less combed. */
IVTC_HD int ivtc_match_rule(const uint32_t *m, int has_prev, int p)
{
    return has_prev && m[2 + p] < m[p] ? IVTC_MATCH_P : IVTC_MATCH_C;
}

/* D: the five difference sums of one cycle; the picture to drop: the smallest, on ties the earliest */
IVTC_HD int ivtc_pick_rule(const uint32_t *D)
{
    int best = 0, k;
    for (k = 1; k < IVTC_CYCLE; k++)
        if (D[k] < D[best]) best = k;
    return best;
}

#endif
