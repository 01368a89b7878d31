"""Decoder output formats (include/dsv1_api.h, csrc/k_pixout.hip) stated in numpy: the definition the GPU is held to.

export() writes packed planar 8-bit frames of subsampling `subsamp` as frames of a tests/_pixfmt.py format dict at subsampling
`out_subsamp`: the chroma planes halved as the reference's conv444to422 / conv422to420 do it (down_chroma), samples widened to the
format's depth (_pixfmt.widen, moved up to bit 15 when msb-aligned), laid out in the format's planes.  Only the bytes of samples are
written into `into`: row padding, the bytes behind the planes and between frames stay as they were -- but for the second luma byte
of the last macro-pixel of an odd-width packed row, which repeats the row's last luma sample."""
import numpy as np

import _cabi as A
import _pixfmt as PF


def allowed_pair(subsamp, out_subsamp):
    """the stream's own subsampling; 4:2:2 from 4:4:4; 4:2:0 from 4:4:4 or 4:2:2"""
    if subsamp not in PF.SUBSAMPS or out_subsamp not in PF.SUBSAMPS:
        return False
    return (out_subsamp == subsamp or (subsamp == A.SUBSAMP_444 and out_subsamp in (A.SUBSAMP_422, A.SUBSAMP_420))
            or (subsamp == A.SUBSAMP_422 and out_subsamp == A.SUBSAMP_420))


def valid(f, w, h, subsamp, out_subsamp):
    return allowed_pair(subsamp, out_subsamp) and PF.plane_layout(f, w, h, out_subsamp) is not None


def halve_h(c):
    """o[y][i] = (c[y][2i] + c[y][min(2i+1, cw-1)] + 1) >> 1, i < (cw+1)/2"""
    c = np.asarray(c, dtype=np.uint8).astype(np.int64)
    i = np.arange((c.shape[1] + 1) // 2)
    return ((c[:, 2 * i] + c[:, np.minimum(2 * i + 1, c.shape[1] - 1)] + 1) >> 1).astype(np.uint8)


def halve_v(c):
    """o[j][x] = (c[2j][x] + c[min(2j+1, ch-1)][x] + 1) >> 1, j < (ch+1)/2"""
    c = np.asarray(c, dtype=np.uint8).astype(np.int64)
    j = np.arange((c.shape[0] + 1) // 2)
    return ((c[2 * j] + c[np.minimum(2 * j + 1, c.shape[0] - 1)] + 1) >> 1).astype(np.uint8)


def down_chroma(c, subsamp, out_subsamp):
    """a chroma plane of a `subsamp` frame at `out_subsamp`: horizontally first, rounded to 8 bits, then vertically"""
    assert allowed_pair(subsamp, out_subsamp)
    if A.hshift(subsamp) != A.hshift(out_subsamp):
        c = halve_h(c)
    if A.vshift(subsamp) != A.vshift(out_subsamp):
        c = halve_v(c)
    return np.asarray(c, dtype=np.uint8)


def planar_at(planar, w, h, subsamp, out_subsamp):
    """[n, frame_bytes at subsamp] -> [n, frame_bytes at out_subsamp] packed planar 8-bit: luma untouched, chroma halved"""
    planar = np.asarray(planar, dtype=np.uint8).reshape(-1, A.frame_bytes(w, h, subsamp))
    out = np.zeros((planar.shape[0], A.frame_bytes(w, h, out_subsamp)), dtype=np.uint8)
    for t in range(planar.shape[0]):
        Y, U, V = PF._split(planar[t], w, h, subsamp)
        u, v = down_chroma(U, subsamp, out_subsamp), down_chroma(V, subsamp, out_subsamp)
        assert u.shape == A.chroma_dims(w, h, out_subsamp)[::-1]
        out[t] = np.concatenate([Y.reshape(-1), u.reshape(-1), v.reshape(-1)])
    return out


def export(planar, f, w, h, subsamp, out_subsamp, n, into=None):
    """planar uint8 [n, frame_bytes(w, h, subsamp)] -> uint8 buffer in format f at out_subsamp: `into` (written in place, at least
    (n - 1) * frame_bytes + the planes long) or a zeroed buffer of n * frame_bytes"""
    assert valid(f, w, h, subsamp, out_subsamp), (f, subsamp, out_subsamp)
    lay, planes, fb = PF.plane_layout(f, w, h, out_subsamp)
    buf = np.zeros(n * fb, dtype=np.uint8) if into is None else into
    assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.size >= (n - 1) * fb + planes
    frames = planar_at(np.asarray(planar).reshape(n, -1), w, h, subsamp, out_subsamp)
    cw, ch = A.chroma_dims(w, h, out_subsamp)
    d = f["depth"]

    def words(v):
        """sample values -> the bytes of their rows"""
        if d == 8:
            return v.astype(np.uint8)
        x = PF.widen(v, d) << ((16 - d) if f["msb"] else 0)
        assert (x < 65536).all()
        x = x.astype("<u2")
        return x.view(np.uint8).reshape(x.shape[:-1] + (-1,))

    for t in range(n):
        Y, U, V = PF._split(frames[t], w, h, out_subsamp)
        if f["layout"] == PF.PLANAR:
            rows = [words(Y), words(U), words(V)]
        elif f["layout"] in (PF.SEMI_UV, PF.SEMI_VU):
            a, b = (U, V) if f["layout"] == PF.SEMI_UV else (V, U)
            rows = [words(Y), words(np.stack([a, b], axis=-1).reshape(ch, 2 * cw))]
        else:
            Yp = np.concatenate([Y, Y[:, -1:]], axis=1)[:, :2 * cw]        # (odd width: the last luma sample once more)
            mp = np.zeros((h, cw, 4), dtype=np.uint8)
            yo, uo = (0, 1) if f["layout"] == PF.YUYV else (1, 0)
            mp[:, :, yo], mp[:, :, yo + 2] = Yp[:, 0::2], Yp[:, 1::2]
            mp[:, :, uo], mp[:, :, uo + 2] = U, V
            rows = [mp.reshape(h, 4 * cw)]
        for (off, pitch, rb, nr), r in zip(lay, rows):
            assert r.shape == (nr, rb), (r.shape, nr, rb)
            for y in range(nr):
                o = t * fb + off + y * pitch
                buf[o:o + rb] = r[y]
    return buf
