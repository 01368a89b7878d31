"""The encoder's SSIM report stated in numpy (include/dsvg.h dsvg_ctx_ssim_enable, csrc/k_quality.hip k_ssim): per plane the sum over
the 8x8 windows at stride 4 of rint(2^32 s), s evaluated in binary64 from the window's integer sums in the kernel's order.  Exact, so
the device's figures must equal it to the integer."""
import numpy as np

import _cabi as A

ONE = 1 << 32
C1, C2 = 26634.24, 239708.16      # (0.01 255)^2 64^2, (0.03 255)^2 64^2


def windows(w, h):
    return ((w - 8) // 4 + 1) * ((h - 8) // 4 + 1) if w >= 8 and h >= 8 else 0


def window_q(sa, sb, sq, sab):
    """rint(2^32 s) of windows with the integer sums given (arrays), as int64"""
    sa, sb, sq, sab = (np.asarray(v, dtype=np.int64) for v in (sa, sb, sq, sab))
    p1, q1 = 2 * sa * sb, sa * sa + sb * sb
    p2, q2 = 2 * (64 * sab - sa * sb), 64 * sq - sa * sa - sb * sb
    f = np.float64
    s = ((p1.astype(f) + C1) * (p2.astype(f) + C2)) / ((q1.astype(f) + C1) * (q2.astype(f) + C2))
    return np.rint(s * float(ONE)).astype(np.int64)


def plane_fx(a, b):
    """SSIM_FX of one plane: a, b uint8 [h, w] (source, reconstruction)"""
    h, w = a.shape
    if not windows(w, h):
        return 0
    bh, bw = h // 4, w // 4
    a = a[:4 * bh, :4 * bw].astype(np.int64)
    b = b[:4 * bh, :4 * bw].astype(np.int64)

    def blocks(x):                          # 4x4 block sums
        return x.reshape(bh, 4, bw, 4).sum(axis=(1, 3))

    def pairs(x):                           # 2x2 groups of blocks: the windows
        return x[:-1, :-1] + x[:-1, 1:] + x[1:, :-1] + x[1:, 1:]
    sums = [pairs(blocks(x)) for x in (a, b, a * a + b * b, a * b)]
    return int(window_q(*sums).sum())


def picture_fx(src, rec, w, h, fmt):
    """[3] SSIM_FX of the planes Y, U, V of one picture (frame bytes of the source and the reconstruction)"""
    cw, ch = A.chroma_dims(w, h, fmt)
    out, o = np.zeros(3, dtype=np.int64), 0
    for p, (pw, ph) in enumerate([(w, h), (cw, ch), (cw, ch)]):
        n = pw * ph
        out[p] = plane_fx(np.asarray(src[o:o + n]).reshape(ph, pw), np.asarray(rec[o:o + n]).reshape(ph, pw))
        o += n
    return out
