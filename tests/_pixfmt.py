"""Source pixel formats (include/dsv1_api.h dsv1_pix_format, csrc/k_pixfmt.hip) stated in numpy: the definition the GPU is held to.

A format is a dict(layout, depth, msb, pitch=(p0, p1, p2), frame_bytes) -- pf() builds one; 0 means tight.  frame_bytes() is
dsv1_pix_frame_bytes (0 = invalid), pack() lays packed planar 8-bit (or wider) frames out in a format with random bytes in every
padding position, convert() is what the device must produce: packed planar 8-bit frames."""
import numpy as np

import _cabi as A

PLANAR, SEMI_UV, SEMI_VU, YUYV, UYVY = 0, 1, 2, 3, 4
LAYOUTS = [PLANAR, SEMI_UV, SEMI_VU, YUYV, UYVY]
DEPTHS = [8, 10, 12, 16]
SUBSAMPS = [A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411]


def pf(layout=PLANAR, depth=8, msb=0, pitch=(0, 0, 0), frame_bytes=0):
    return dict(layout=layout, depth=depth, msb=msb, pitch=tuple(pitch), frame_bytes=frame_bytes)


def valid(layout, depth, fmt):
    if layout not in LAYOUTS or depth not in DEPTHS or fmt not in SUBSAMPS:
        return False
    if layout in (SEMI_UV, SEMI_VU):
        return fmt in (A.SUBSAMP_420, A.SUBSAMP_422)
    if layout in (YUYV, UYVY):
        return fmt == A.SUBSAMP_422 and depth == 8
    return True


def source_planes(f, w, h, fmt):
    """[(row bytes, rows)] of the format's source planes, or None for an invalid combination"""
    if w < 1 or h < 1 or not valid(f["layout"], f["depth"], fmt):
        return None
    if f["depth"] > 8 and f["msb"] not in (0, 1):
        return None
    cw, ch = A.chroma_dims(w, h, fmt)
    b = 2 if f["depth"] > 8 else 1
    if f["layout"] == PLANAR:
        return [(w * b, h), (cw * b, ch), (cw * b, ch)]
    if f["layout"] in (SEMI_UV, SEMI_VU):
        return [(w * b, h), (2 * cw * b, ch)]
    return [(4 * cw, h)]


def plane_layout(f, w, h, fmt):
    """([(offset, pitch, row bytes, rows)], bytes of the planes, frame stride) or None"""
    sp = source_planes(f, w, h, fmt)
    if sp is None:
        return None
    out, off = [], 0
    for k, (rb, rows) in enumerate(sp):
        p = f["pitch"][k]
        if p < 0 or (p and p < rb):
            return None
        p = p or rb
        out.append((off, p, rb, rows))
        off += p * rows
    if f["frame_bytes"] and f["frame_bytes"] < off:
        return None
    return out, off, f["frame_bytes"] or off


def frame_bytes(f, w, h, fmt):
    lay = plane_layout(f, w, h, fmt)
    return 0 if lay is None else lay[2]


def reduce_depth(x, depth, msb):
    """16-bit words -> 8 bits: v = msb ? x >> (16 - d) : x & (2^d - 1); min(255, (v + 2^(d-9)) >> (d - 8))"""
    x = np.asarray(x, dtype=np.uint16).astype(np.int64)
    v = (x >> (16 - depth)) if msb else (x & ((1 << depth) - 1))
    return np.minimum(255, (v + (1 << (depth - 9))) >> (depth - 8)).astype(np.uint8)


def _split(frame, w, h, fmt):
    cw, ch = A.chroma_dims(w, h, fmt)
    frame = np.asarray(frame).reshape(-1)
    return frame[:w * h].reshape(h, w), frame[w * h:w * h + cw * ch].reshape(ch, cw), frame[w * h + cw * ch:w * h + 2 * cw * ch].reshape(ch, cw)


def pack(planar, f, w, h, fmt, rng=None, garbage=True):
    """planar: [n, samples per frame] packed planar frames whose samples are the VALUES v (uint8 for depth 8, else integers below
    2^depth) -> uint8 [n * frame_bytes] in format f.  Padding bytes, the unused luma of an odd packed row and (garbage) the unused
    bits of every 16-bit word are random."""
    rng = rng or np.random.default_rng(1)
    lay, _, fb = plane_layout(f, w, h, fmt)
    planar = np.asarray(planar)
    n, d, wide = planar.shape[0], f["depth"], f["depth"] > 8
    buf = rng.integers(0, 256, n * fb, dtype=np.uint8)
    cw, ch = A.chroma_dims(w, h, fmt)

    def words(v):
        """sample values -> the bytes of their row(s)"""
        if not wide:
            return v.astype(np.uint8)
        v = v.astype(np.uint32)
        junk = rng.integers(0, 1 << 16, v.shape, dtype=np.uint32) if garbage else np.zeros(v.shape, dtype=np.uint32)
        x = ((v << (16 - d)) | (junk & ((1 << (16 - d)) - 1))) if f["msb"] else (v | (junk & ~np.uint32((1 << d) - 1) & 0xFFFF))
        x = x.astype("<u2")
        return x.view(np.uint8).reshape(x.shape[:-1] + (-1,))

    for t in range(n):
        Y, U, V = _split(planar[t], w, h, fmt)
        if f["layout"] == PLANAR:
            rows = [words(Y), words(U), words(V)]
        elif f["layout"] in (SEMI_UV, SEMI_VU):
            a, b = (U, V) if f["layout"] == SEMI_UV else (V, U)
            rows = [words(Y), words(np.stack([a, b], axis=-1).reshape(ch, 2 * cw))]
        else:
            Yp = rng.integers(0, 256, (h, 2 * cw), dtype=np.uint8)
            Yp[:, :w] = Y
            mp = np.zeros((h, cw, 4), dtype=np.uint8)
            yo, uo = (0, 1) if f["layout"] == YUYV else (1, 0)
            mp[:, :, yo], mp[:, :, yo + 2] = Yp[:, 0::2], Yp[:, 1::2]
            mp[:, :, uo], mp[:, :, uo + 2] = U, V
            rows = [mp.reshape(h, 4 * cw)]
        for (off, pitch, rb, nr), r in zip(lay, rows):
            assert r.shape == (nr, rb), (r.shape, nr, rb)
            for y in range(nr):
                o = t * fb + off + y * pitch
                buf[o:o + rb] = r[y]
    return buf


def convert(buf, f, w, h, fmt, n):
    """uint8 [>= (n - 1) * frame_bytes + planes] in format f -> uint8 [n, frame_bytes of packed planar 8-bit]"""
    lay, _, fb = plane_layout(f, w, h, fmt)
    buf = np.asarray(buf).view(np.uint8).reshape(-1)
    cw, ch = A.chroma_dims(w, h, fmt)
    wide = f["depth"] > 8
    out = np.zeros((n, A.frame_bytes(w, h, fmt)), dtype=np.uint8)

    def samples(t, k):
        off, pitch, rb, nr = lay[k]
        r = np.stack([buf[t * fb + off + y * pitch: t * fb + off + y * pitch + rb] for y in range(nr)])
        if not wide:
            return r
        return reduce_depth(np.ascontiguousarray(r).view("<u2"), f["depth"], f["msb"])

    for t in range(n):
        if f["layout"] == PLANAR:
            Y, U, V = samples(t, 0), samples(t, 1), samples(t, 2)
        elif f["layout"] in (SEMI_UV, SEMI_VU):
            Y, C2 = samples(t, 0), samples(t, 1).reshape(ch, cw, 2)
            U, V = (C2[:, :, 0], C2[:, :, 1]) if f["layout"] == SEMI_UV else (C2[:, :, 1], C2[:, :, 0])
        else:
            mp = samples(t, 0).reshape(h, cw, 4)
            yo, uo = (0, 1) if f["layout"] == YUYV else (1, 0)
            Y = np.stack([mp[:, :, yo], mp[:, :, yo + 2]], axis=-1).reshape(h, 2 * cw)[:, :w]
            U, V = mp[:, :, uo], mp[:, :, uo + 2]
        out[t] = np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)])
    return out


def widen(planar8, depth):
    """8-bit sample values at depth d: x << (d - 8) (convert() of their pack() gives planar8 back)"""
    return np.asarray(planar8, dtype=np.uint32) << (depth - 8)
