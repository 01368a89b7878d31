"""Chroma resampling in the source and output passes (include/dsv1_api.h, chroma resampling; csrc/k_pixfmt.hip, csrc/k_pixout.hip)
stated in numpy: the definition the GPU is held to.  No arithmetic of its own: the halving on the way in is tests/_pixout.py's
(conv444to422 / conv422to420) behind tests/_pixfmt.py's conversion, the doubling on the way out is tests/_rgb.py's upsample() in
front of tests/_pixout.py's export at the output's own subsampling."""
import numpy as np

import _cabi as A
import _pixfmt as PF
import _pixout as PO
import _rgb as RGB

REPLICATE, LINEAR = RGB.REPLICATE, RGB.LINEAR
MODES = [REPLICATE, LINEAR]
HALVING = [(A.SUBSAMP_444, A.SUBSAMP_422), (A.SUBSAMP_444, A.SUBSAMP_420), (A.SUBSAMP_422, A.SUBSAMP_420)]
DOUBLING = [(b, a) for a, b in HALVING]


def valid_in(f, w, h, src_subsamp, subsamp):
    """a source of format f at src_subsamp into frames at subsamp: the same subsampling or a halving pair, and the layout valid at
    src_subsamp"""
    if src_subsamp not in PF.SUBSAMPS or subsamp not in PF.SUBSAMPS:
        return False
    return (src_subsamp == subsamp or (src_subsamp, subsamp) in HALVING) and PF.plane_layout(f, w, h, src_subsamp) is not None


def valid_out(f, w, h, subsamp, out_subsamp, mode):
    """frames at subsamp written as format f at out_subsamp: a known mode, a pair the output pass takes already or a doubling pair,
    and the layout valid at out_subsamp"""
    if mode not in MODES:
        return False
    return (PO.allowed_pair(subsamp, out_subsamp) or (subsamp, out_subsamp) in DOUBLING) and PF.plane_layout(f, w, h, out_subsamp) is not None


def convert_sub(buf, f, w, h, src_subsamp, subsamp, n):
    """uint8 buffer of n frames in format f at src_subsamp -> uint8 [n, frame_bytes(w, h, subsamp)] packed planar 8-bit: reduced to 8
    bits, then halved"""
    assert valid_in(f, w, h, src_subsamp, subsamp), (f, src_subsamp, subsamp)
    return PO.planar_at(PF.convert(buf, f, w, h, src_subsamp, n), w, h, src_subsamp, subsamp)


def up_chroma(c, w, h, subsamp, out_subsamp, mode):
    """a chroma plane of a w x h frame at subsamp on the chroma grid of out_subsamp: tests/_rgb.py's upsample() with the output's chroma
    dims for the luma grid and the shifts that drop for the plane's"""
    dh, dv = A.hshift(subsamp) - A.hshift(out_subsamp), A.vshift(subsamp) - A.vshift(out_subsamp)
    assert dh in (0, 1) and dv in (0, 1)
    ocw, och = A.chroma_dims(w, h, out_subsamp)
    return RGB.upsample(c, ocw, och, (dh << 2) | dv, mode).astype(np.uint8)


def planar_up(planar, w, h, subsamp, out_subsamp, mode):
    """[n, frame_bytes at subsamp] -> [n, frame_bytes at out_subsamp] packed planar 8-bit: luma untouched, chroma doubled"""
    assert (subsamp, out_subsamp) in DOUBLING and mode in MODES
    planar = np.asarray(planar, dtype=np.uint8).reshape(-1, A.frame_bytes(w, h, subsamp))
    out = np.zeros((planar.shape[0], A.frame_bytes(w, h, out_subsamp)), dtype=np.uint8)
    for t in range(planar.shape[0]):
        Y, U, V = PF._split(planar[t], w, h, subsamp)
        u, v = up_chroma(U, w, h, subsamp, out_subsamp, mode), up_chroma(V, w, h, subsamp, out_subsamp, mode)
        assert u.shape == A.chroma_dims(w, h, out_subsamp)[::-1]
        out[t] = np.concatenate([Y.reshape(-1), u.reshape(-1), v.reshape(-1)])
    return out


def export_up(planar, f, w, h, subsamp, out_subsamp, mode, n, into=None):
    """planar uint8 [n, frame_bytes(w, h, subsamp)] -> uint8 buffer in format f at out_subsamp (tests/_pixout.py export(): `into` or a
    zeroed buffer; only the bytes of samples are written); `mode` is read only where chroma goes up"""
    assert valid_out(f, w, h, subsamp, out_subsamp, mode), (f, subsamp, out_subsamp, mode)
    if (subsamp, out_subsamp) not in DOUBLING:
        return PO.export(planar, f, w, h, subsamp, out_subsamp, n, into=into)
    return PO.export(planar_up(np.asarray(planar).reshape(n, -1), w, h, subsamp, out_subsamp, mode), f, w, h, out_subsamp, out_subsamp, n, into=into)
