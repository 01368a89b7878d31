"""The levels pass and the histogram (include/dsv1_api.h, Levels) stated in numpy: the table builders in exact rationals
(fractions.Fraction, no floating point and none of the library's integer tricks), the pass, the histogram, the range and the point
rules, and the case lists the levels tests share."""
from fractions import Fraction
from math import floor

import numpy as np

import _cabi as A

FORMATS = (A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411)
SMALL = [(1, 1), (17, 3), (33, 9), (70, 50)]             # 17 x 3 at 4:2:0 is 87 bytes a frame: boundaries fall inside 16-byte chunks
BIG = (1920, 1080)


def r(a, b):
    """the exact rational a / b rounded half up"""
    return floor(Fraction(a, b) + Fraction(1, 2))


def clamp(v):
    return min(255, max(0, v))


def identity():
    return np.tile(np.arange(256, dtype=np.uint8), (3, 1))


def range_(src_full, dst_full):
    """[3][256] uint8, or None for flags that are none"""
    if src_full not in (0, 1) or dst_full not in (0, 1):
        return None
    if src_full == dst_full:
        return identity()
    t = np.zeros((3, 256), dtype=np.uint8)
    for v in range(256):
        if src_full:
            y, c = 16 + r(v * 219, 255), 128 + r((v - 128) * 224, 255)
            assert 0 <= y <= 255 and 0 <= c <= 255
        else:
            y, c = clamp(r((v - 16) * 255, 219)), clamp(128 + r((v - 128) * 255, 224))
        t[0, v], t[1, v], t[2, v] = y, c, c
    return t


def adjust_valid(ib, iw, ob, ow, sat):
    return 0 <= ib < iw <= 255 and 0 <= ob <= ow <= 255 and 0 <= sat <= 1024


def adjust(ib, iw, ob, ow, sat):
    if not adjust_valid(ib, iw, ob, ow, sat):
        return None
    t = np.zeros((3, 256), dtype=np.uint8)
    for v in range(256):
        t[0, v] = ob if v <= ib else ow if v >= iw else ob + r((v - ib) * (ow - ob), iw - ib)
        t[1, v] = t[2, v] = clamp(128 + r((v - 128) * sat, 256))
    return t


def compose(a, b):
    """a first"""
    return np.stack([b[p][a[p]] for p in range(3)])


def plane_bounds(w, h, fmt):
    cw, ch = A.chroma_dims(w, h, fmt)
    return [0, w * h, w * h + cw * ch, w * h + 2 * cw * ch]


def levels_clip(clip, w, h, fmt, t):
    e = plane_bounds(w, h, fmt)
    clip = np.asarray(clip, dtype=np.uint8).reshape(-1, e[3])
    out = np.empty_like(clip)
    for p in range(3):
        out[:, e[p]:e[p + 1]] = np.asarray(t[p], dtype=np.uint8)[clip[:, e[p]:e[p + 1]]]
    return out


def histogram(clip, w, h, fmt):
    """uint32 [n][3][256]"""
    e = plane_bounds(w, h, fmt)
    clip = np.asarray(clip, dtype=np.uint8).reshape(-1, e[3])
    return np.array([[np.bincount(f[e[p]:e[p + 1]], minlength=256) for p in range(3)] for f in clip], dtype=np.uint32)


def range_from_histogram(hist, ppm):
    g = np.asarray(hist).reshape(-1, 3, 256).astype(object).sum(axis=0)        # (Python integers: no overflow)
    outside = sum(int(g[0][v]) for v in range(256) if v < 16 or v > 235) + sum(int(g[p][v]) for p in (1, 2) for v in range(256) if v < 16 or v > 240)
    total = sum(int(x) for x in g.reshape(-1))
    return outside * 1000000 > ppm * total


def points_from_histogram(hist, low_ppm, high_ppm):
    """(black, white) or None"""
    y = [int(x) for x in np.asarray(hist).reshape(-1, 3, 256).astype(object).sum(axis=0)[0]]
    total = sum(y)
    black = max(b for b in range(256) if sum(y[:b]) * 1000000 <= low_ppm * total)
    white = min(w for w in range(256) if sum(y[w + 1:]) * 1000000 <= high_ppm * total)
    return (black, white) if black < white else None


def noise(n, w, h, fmt, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, A.frame_bytes(w, h, fmt)), dtype=np.uint8)


def random_tables(seed):
    """three different tables, none a permutation of another's rows: a table applied to the wrong plane shows"""
    return np.random.default_rng(seed).integers(0, 256, size=(3, 256), dtype=np.uint8)
