"""RGB in and out (include/dsv1_api.h, RGB; csrc/k_rgb.hip) stated in numpy: the definition the GPU is held to.  Written from the
definition -- Kr, Kb, the ranges, round half up -- not from the kernels: tables() derives the integer tables in exact rationals,
to_ycc() / to_rgb() are the per-pixel arithmetic in int64, halve() the source subsampling (tests/_pixout.py: the decoder output
pass's rule), upsample() the two ways chroma reaches the luma grid, pack() / unpack() the memory layouts.  import_() and export()
put them together; export() writes only the bytes of pixels into `into`."""
from fractions import Fraction as Fr

import numpy as np

import _cabi as A
import _pixout as PO

RGB24, BGR24, RGBA, BGRA, ARGB, ABGR, PLANAR_RGB, PLANAR_GBR = range(8)
ORDERS = list(range(8))
NAMES = ["RGB24", "BGR24", "RGBA", "BGRA", "ARGB", "ABGR", "PLANAR_RGB", "PLANAR_GBR"]
BT601, BT709, BT2020 = 0, 1, 2
MATRICES = [BT601, BT709, BT2020]
REPLICATE, LINEAR = 0, 1
SUBSAMPS = [A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420]
K = {BT601: (Fr(299, 1000), Fr(114, 1000)), BT709: (Fr(2126, 10000), Fr(722, 10000)), BT2020: (Fr(2627, 10000), Fr(593, 10000))}
# memory position -> component (0 R, 1 G, 2 B); the byte of a 4-byte pixel that holds A
COMP = {RGB24: (0, 1, 2), BGR24: (2, 1, 0), RGBA: (0, 1, 2), BGRA: (2, 1, 0), ARGB: (0, 1, 2), ABGR: (2, 1, 0), PLANAR_RGB: (0, 1, 2), PLANAR_GBR: (1, 2, 0)}
ALPHA = {RGBA: 3, BGRA: 3, ARGB: 0, ABGR: 0}


def rf(order=RGB24, matrix=BT709, full=0, upsample=LINEAR, pitch=(0, 0, 0), frame_bytes=0):
    return dict(order=order, matrix=matrix, full=full, upsample=upsample, pitch=tuple(pitch), frame_bytes=frame_bytes)


def r(x):
    """an exact rational rounded half up"""
    x = Fr(x)
    return (2 * x.numerator + x.denominator) // (2 * x.denominator)


def ranges(full):
    """sy, sc, oy"""
    return (Fr(1), Fr(1), 0) if full else (Fr(219, 255), Fr(224, 255), 16)


def tables(matrix, full):
    """(forward Q16 [3][3] rows Y, Cb, Cr over R, G, B; inverse Q14 IY, RV, GU, GV, BU), python ints"""
    kr, kb = K[matrix]
    kg = 1 - kr - kb
    sy, sc, _ = ranges(full)
    yr, yb = r(65536 * sy * kr), r(65536 * sy * kb)
    hf = r(65536 * sc / 2)
    cbr = -r(65536 * sc * kr / (2 * (1 - kb)))
    crb = -r(65536 * sc * kb / (2 * (1 - kr)))
    fwd = [[yr, r(65536 * sy) - yr - yb, yb], [cbr, -(hf + cbr), hf], [hf, -(hf + crb), crb]]
    inv = [r(16384 / sy), r(16384 * 2 * (1 - kr) / sc), -r(16384 * 2 * (1 - kb) * kb / (kg * sc)), -r(16384 * 2 * (1 - kr) * kr / (kg * sc)),
           r(16384 * 2 * (1 - kb) / sc)]
    return fwd, inv


def to_ycc(R, G, B, matrix, full, clamp=True):
    """per pixel, 4:4:4: int64 arrays (before the clamp when clamp=False)"""
    fwd, _ = tables(matrix, full)
    oy = ranges(full)[2]
    R, G, B = (np.asarray(x).astype(np.int64) for x in (R, G, B))
    out = []
    for row, off in zip(fwd, (oy, 128, 128)):
        v = (row[0] * R + row[1] * G + row[2] * B + (off << 16) + 32768) >> 16
        out.append(np.clip(v, 0, 255) if clamp else v)
    return out


def to_rgb(Y, Cb, Cr, matrix, full):
    """per pixel, chroma on the luma grid: int64 arrays 0..255"""
    _, (IY, RV, GU, GV, BU) = tables(matrix, full)
    oy = ranges(full)[2]
    y, u, v = np.asarray(Y).astype(np.int64) - oy, np.asarray(Cb).astype(np.int64) - 128, np.asarray(Cr).astype(np.int64) - 128
    return [np.clip((IY * y + RV * v + 8192) >> 14, 0, 255), np.clip((IY * y + GU * u + GV * v + 8192) >> 14, 0, 255),
            np.clip((IY * y + BU * u + 8192) >> 14, 0, 255)]


def halve(c, subsamp):
    """an 8-bit 4:4:4 chroma plane at `subsamp`: the decoder output pass's rule"""
    return PO.down_chroma(c, A.SUBSAMP_444, subsamp)


def up_v(c, h):
    c = np.asarray(c).astype(np.int64)
    ch = c.shape[0]
    j = np.arange(ch)
    o = np.zeros((2 * ch, c.shape[1]), dtype=np.int64)
    o[0::2] = (3 * c + c[np.maximum(j - 1, 0)] + 2) >> 2
    o[1::2] = (3 * c + c[np.minimum(j + 1, ch - 1)] + 2) >> 2
    return o[:h]


def upsample(c, w, h, subsamp, mode):
    """a chroma plane of a `subsamp` frame on the w x h luma grid"""
    hs, vs = A.hshift(subsamp), A.vshift(subsamp)
    c = np.asarray(c).astype(np.int64)
    if mode == REPLICATE:
        return c[np.arange(h) >> vs][:, np.arange(w) >> hs]
    if vs:
        c = up_v(c, h)
    if hs:
        c = up_v(c.T, w).T
    assert c.shape == (h, w)
    return c


def layout(f, w, h):
    """([(offset, pitch, row bytes)] per plane, planes' end, frame to frame) or None for an invalid format"""
    if f["order"] not in ORDERS or f["matrix"] not in MATRICES or f["full"] not in (0, 1) or f["upsample"] not in (REPLICATE, LINEAR) or w < 1 or h < 1:
        return None
    planar = f["order"] >= PLANAR_RGB
    rb = w * (1 if planar else 3 if f["order"] <= BGR24 else 4)
    lay, off = [], 0
    for p in range(3 if planar else 1):
        pitch = f["pitch"][p]
        if pitch < 0 or (pitch and pitch < rb):
            return None
        pitch = pitch or rb
        lay.append((off, pitch, rb))
        off += pitch * h
    if f["frame_bytes"] and f["frame_bytes"] < off:
        return None
    return lay, off, f["frame_bytes"] or off


def frame_bytes(f, w, h):
    L = layout(f, w, h)
    return L[2] if L else 0


def rows_of(f, R, G, B):
    """the planes' rows of one frame: list of [h, row bytes] uint8"""
    comp = [np.asarray(x).astype(np.uint8) for x in (R, G, B)]
    mem = [comp[k] for k in COMP[f["order"]]]
    if f["order"] >= PLANAR_RGB:
        return mem
    h, w = comp[0].shape
    if f["order"] <= BGR24:
        return [np.stack(mem, axis=-1).reshape(h, 3 * w)]
    a = ALPHA[f["order"]]
    px = np.full((h, w, 4), 255, dtype=np.uint8)
    for k in range(3):
        px[:, :, k + (1 if a == 0 else 0)] = mem[k]
    return [px.reshape(h, 4 * w)]


def pack(R, G, B, f, w, h, rng, alpha=None):
    """[n, h, w] components -> the raw clip, padding (and A) random"""
    n = R.shape[0]
    lay, planes, fb = layout(f, w, h)
    buf = rng.integers(0, 256, n * fb, dtype=np.uint8)
    for t in range(n):
        rows = rows_of(f, R[t], G[t], B[t])
        if f["order"] in ALPHA:
            rows[0].reshape(h, w, 4)[:, :, ALPHA[f["order"]]] = rng.integers(0, 256, (h, w), dtype=np.uint8)
        for (off, pitch, rb), rr in zip(lay, rows):
            for y in range(h):
                o = t * fb + off + y * pitch
                buf[o:o + rb] = rr[y]
    return buf


def unpack(buf, f, w, h, n):
    """the raw clip -> R, G, B [n, h, w] uint8: only the bytes of pixels are looked at"""
    lay, planes, fb = layout(f, w, h)
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    out = np.zeros((3, n, h, w), dtype=np.uint8)
    for t in range(n):
        planes_ = [np.stack([buf[t * fb + off + y * pitch:t * fb + off + y * pitch + rb] for y in range(h)]) for off, pitch, rb in lay]
        if f["order"] >= PLANAR_RGB:
            mem = planes_
        elif f["order"] <= BGR24:
            mem = [planes_[0].reshape(h, w, 3)[:, :, k] for k in range(3)]
        else:
            s = 1 if ALPHA[f["order"]] == 0 else 0
            mem = [planes_[0].reshape(h, w, 4)[:, :, k + s] for k in range(3)]
        for k in range(3):
            out[COMP[f["order"]][k], t] = mem[k]
    return out[0], out[1], out[2]


def import_(buf, f, w, h, subsamp, n):
    """raw RGB clip -> uint8 [n, frame_bytes(w, h, subsamp)] packed planar"""
    assert subsamp in SUBSAMPS and layout(f, w, h) is not None
    R, G, B = unpack(buf, f, w, h, n)
    out = np.zeros((n, A.frame_bytes(w, h, subsamp)), dtype=np.uint8)
    for t in range(n):
        Y, Cb, Cr = to_ycc(R[t], G[t], B[t], f["matrix"], f["full"])
        u, v = halve(Cb.astype(np.uint8), subsamp), halve(Cr.astype(np.uint8), subsamp)
        assert u.shape == A.chroma_dims(w, h, subsamp)[::-1]
        out[t] = np.concatenate([Y.astype(np.uint8).reshape(-1), u.reshape(-1), v.reshape(-1)])
    return out


def split(frame, w, h, subsamp):
    cw, ch = A.chroma_dims(w, h, subsamp)
    frame = np.asarray(frame, dtype=np.uint8).reshape(-1)
    return frame[:w * h].reshape(h, w), frame[w * h:w * h + cw * ch].reshape(ch, cw), frame[w * h + cw * ch:w * h + 2 * cw * ch].reshape(ch, cw)


def export(planar, f, w, h, subsamp, n, into=None):
    """planar uint8 [n, frame_bytes(w, h, subsamp)] -> RGB frames of f: `into` (written in place, at least (n - 1) * frame_bytes + the
    planes long) or a zeroed buffer of n * frame_bytes.  Only the bytes of pixels are written (A: 255)."""
    assert subsamp in SUBSAMPS
    lay, planes, fb = layout(f, w, h)
    buf = np.zeros(n * fb, dtype=np.uint8) if into is None else into
    assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.size >= (n - 1) * fb + planes
    planar = np.asarray(planar, dtype=np.uint8).reshape(n, -1)
    for t in range(n):
        Y, U, V = split(planar[t], w, h, subsamp)
        u, v = upsample(U, w, h, subsamp, f["upsample"]), upsample(V, w, h, subsamp, f["upsample"])
        R, G, B = to_rgb(Y, u, v, f["matrix"], f["full"])
        for (off, pitch, rb), rr in zip(lay, rows_of(f, R, G, B)):
            for y in range(h):
                o = t * fb + off + y * pitch
                buf[o:o + rb] = rr[y]
    return buf
