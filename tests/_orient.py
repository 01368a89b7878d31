"""The orientation pass (include/dsv1_api.h, Orientation) stated in numpy, the algebra of its eight codes, and the case lists the
orientation tests share.  A code is a bit set: bit 2 transposes first, bit 0 then mirrors the columns of the result, bit 1 its rows."""
import numpy as np

import _cabi as A

NONE, HFLIP, VFLIP, ROT180, TRANSPOSE, ROT90, ROT270, TRANSVERSE = range(8)
NAMES = ("none", "hflip", "vflip", "rot180", "transpose", "rot90", "rot270", "transverse")
FORMATS = (A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411)
EXIF = {1: NONE, 2: HFLIP, 3: ROT180, 4: VFLIP, 5: TRANSPOSE, 6: ROT90, 7: TRANSVERSE, 8: ROT270}
TILE = (128, 64)                                          # k_orient_tr's tile: input rows x input columns


def valid(orient, fmt):
    """the predicate of include/dsv1_api.h"""
    if orient not in range(8) or fmt not in FORMATS:
        return False
    return not (orient & 4) or A.hshift(fmt) == A.vshift(fmt)


def dims(orient, w, h):
    """(ow, oh) of the luma, or None for a code that is none"""
    if orient not in range(8) or w < 1 or h < 1:
        return None
    return (h, w) if orient & 4 else (w, h)


def plane(i, orient):
    """one plane: the table of the header, entry by entry (fancy indexing on the formula, not numpy's own flips)"""
    i = np.asarray(i)
    ih, iw = i.shape
    oh, ow = (iw, ih) if orient & 4 else (ih, iw)
    y, x = np.mgrid[0:oh, 0:ow]
    rows, cols = {NONE: (y, x), HFLIP: (y, iw - 1 - x), VFLIP: (ih - 1 - y, x), ROT180: (ih - 1 - y, iw - 1 - x),
                  TRANSPOSE: (x, y), ROT90: (ih - 1 - x, y), ROT270: (x, iw - 1 - y), TRANSVERSE: (ih - 1 - x, iw - 1 - y)}[orient]
    return i[rows, cols]


def planes(frame, w, h, fmt):
    """the three planes of one packed planar frame as 2-D views"""
    cw, ch = A.chroma_dims(w, h, fmt)
    f = np.asarray(frame).reshape(-1)
    return [f[:w * h].reshape(h, w), f[w * h:w * h + cw * ch].reshape(ch, cw), f[w * h + cw * ch:w * h + 2 * cw * ch].reshape(ch, cw)]


def orient_clip(clip, w, h, fmt, orient):
    """[n][frame bytes of w x h] -> [n][frame bytes of dims(orient, w, h)], every plane on its own at its own dimensions"""
    assert valid(orient, fmt)
    fb = A.frame_bytes(w, h, fmt)
    ow, oh = dims(orient, w, h)
    assert A.frame_bytes(ow, oh, fmt) == fb
    clip = np.asarray(clip, dtype=np.uint8).reshape(-1, fb)
    out = np.zeros_like(clip)
    for t in range(clip.shape[0]):
        for i, o in zip(planes(clip[t], w, h, fmt), planes(out[t], ow, oh, fmt)):
            o[...] = plane(i, orient)
    return out


def compose(a, b):
    """the code equal to a and then b, found by trying: the codes are told apart by what they do to a 2 x 3 array of distinct values"""
    probe = np.arange(6).reshape(2, 3)
    got = plane(plane(probe, a), b)
    (c,) = [k for k in range(8) if plane(probe, k).shape == got.shape and np.array_equal(plane(probe, k), got)]
    return c


def inverse(a):
    (c,) = [k for k in range(8) if compose(a, k) == NONE]
    return c


def place_by_matrix(i, m):
    """the samples of plane i placed where the display matrix m (9 entries, 16.16) shows them, re-based to zero"""
    a, b, c, d = (v // 65536 for v in (m[0], m[1], m[3], m[4]))
    ih, iw = i.shape
    q, p = np.mgrid[0:ih, 0:iw]
    X, Y = a * p + c * q, b * p + d * q
    X, Y = X - X.min(), Y - Y.min()
    out = np.full((Y.max() + 1, X.max() + 1), -1, dtype=np.int64)
    out[Y, X] = i
    return out


def matrix(a, b, c, d, tx=0, ty=0, u=0, v=0, w=1 << 30):
    one = 65536
    return [a * one, b * one, u, c * one, d * one, v, tx, ty, w]


MATRICES = {NONE: (1, 0, 0, 1), HFLIP: (-1, 0, 0, 1), VFLIP: (1, 0, 0, -1), ROT180: (-1, 0, 0, -1),
            TRANSPOSE: (0, 1, 1, 0), ROT90: (0, 1, -1, 0), ROT270: (0, -1, 1, 0), TRANSVERSE: (0, -1, -1, 0)}       # (a, b, c, d)


def noise(n, w, h, fmt, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, A.frame_bytes(w, h, fmt)), dtype=np.uint8)


# ---- GPU cases: a tile's last partial column and row, a plane smaller than one tile, rows of every alignment mod 16 ----
GEOMS = [(1, 1), (1, 9), (9, 1), (3, 5), (16, 16), (63, 65), (64, 64), (65, 63), (70, 50), (127, 129), (129, 127), (250, 130)]
for T in TILE:
    if T not in (64, 128):
        GEOMS += [(T - 1, T + 1), (T + 1, T - 1)]

