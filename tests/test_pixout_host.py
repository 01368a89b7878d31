"""Decoder output formats on the host (no GPU): the numpy statement tests/_pixout.py against the library's host conv444to422 /
conv422to420 (and the compiled reference's, where it exists), against tests/_pixfmt.py (converting an exported clip gives the
planar frames back), and the validity table of dsv1_export_clip / dsv1_decbatch_set_output_format, which is decided before any
device is looked at."""
import ctypes as C
import importlib
import itertools

import numpy as np
import pytest

import _cabi as A
import _pixfmt as PF
import _pixout as PO

DSVG_ERR_ARG = -2
NODEV = 1 << 20          # a device number no machine has: a call that passes the checks fails there, not with DSVG_ERR_ARG
PLANES = [(16, 16), (17, 9), (1, 1), (2, 5), (33, 1)]       # chroma planes w x h: odd sizes exercise both clamps


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("digital-subband-video-1_amd")


def cpf(pkg, f):
    return pkg.PixFormat(f["layout"], f["depth"], f["msb"], f["pitch"], f["frame_bytes"])


def c_conv(L, name, src, dw, dh):
    """conv444to422 / conv422to420 of library L on one plane (destination stride beyond its width: nothing else is written)"""
    src = np.ascontiguousarray(src, dtype=np.uint8)
    stride = dw + 3
    dst = np.full((dh, stride), 0xEE, dtype=np.uint8)
    ps = A.Plane(A.u8p(src), src.size, 0, src.shape[1], src.shape[1], src.shape[0], 0, 0)
    pd = A.Plane(A.u8p(dst), dst.size, 0, stride, dw, dh, 0, 0)
    fn = getattr(L, name)
    fn.restype = None
    fn.argtypes = [C.POINTER(A.Plane), C.POINTER(A.Plane)]
    fn(C.byref(ps), C.byref(pd))
    assert (dst[:, dw:] == 0xEE).all()
    return dst[:, :dw].copy()


def check_against(L):
    for k, (w, h) in enumerate(PLANES):
        c = np.random.default_rng(100 + k).integers(0, 256, (h, w), dtype=np.uint8)
        c[-1, -1], c[0, 0] = 255, 255                    # (255 + 255 + 1 must not wrap)
        hw, hh = (w + 1) // 2, (h + 1) // 2
        h422 = PO.down_chroma(c, A.SUBSAMP_444, A.SUBSAMP_422)
        assert h422.shape == (h, hw) and np.array_equal(h422, c_conv(L, "conv444to422", c, hw, h)), (w, h)
        v420 = PO.down_chroma(c, A.SUBSAMP_422, A.SUBSAMP_420)
        assert v420.shape == (hh, w) and np.array_equal(v420, c_conv(L, "conv422to420", c, w, hh)), (w, h)
        both = PO.down_chroma(c, A.SUBSAMP_444, A.SUBSAMP_420)
        assert both.shape == (hh, hw) and np.array_equal(both, c_conv(L, "conv422to420", c_conv(L, "conv444to422", c, hw, h), hw, hh)), (w, h)
        assert np.array_equal(PO.down_chroma(c, A.SUBSAMP_420, A.SUBSAMP_420), c)


def test_down_chroma_equals_the_librarys_host_functions(pkg):
    check_against(pkg.lib())


def test_down_chroma_equals_the_reference(ref):
    check_against(ref)


@pytest.mark.parametrize("w,h", [(36, 20), (35, 19), (17, 9), (1, 1), (2, 5), (33, 1)])
def test_output_chroma_dims_are_rshift_up_of_the_luma_dims(w, h):
    for fmt, ofmt in itertools.product(PF.SUBSAMPS, PF.SUBSAMPS):
        if not PO.allowed_pair(fmt, ofmt):
            continue
        x = np.random.default_rng(w + h).integers(0, 256, (1, A.frame_bytes(w, h, fmt)), dtype=np.uint8)
        out = PO.planar_at(x, w, h, fmt, ofmt)           # (asserts the plane dims)
        assert out.shape == (1, A.frame_bytes(w, h, ofmt))
        assert np.array_equal(out[0, :w * h], x[0, :w * h])          # luma untouched


def paddings(f, w, h, fmt):
    lay, planes, _ = PF.plane_layout(f, w, h, fmt)
    pitch = tuple(lay[k][2] + (5, 16, 7)[k] if k < len(lay) else 0 for k in range(3))
    return [f, dict(f, pitch=pitch, frame_bytes=PF.plane_layout(dict(f, pitch=pitch), w, h, fmt)[1] + 37)]


def formats():
    for layout, depth, msb in itertools.product(PF.LAYOUTS, PF.DEPTHS, (0, 1)):
        if depth > 8 or not msb:
            yield PF.pf(layout, depth, msb)


@pytest.mark.parametrize("w,h", [(36, 20), (35, 19)])
def test_round_trip(w, h):
    """_pixfmt.convert(_pixout.export(x)) == x for every valid format at the stream's own subsampling, tight and padded; the padding
    of the buffer exported into is untouched"""
    rng = np.random.default_rng(w * h)
    ncases = 0
    for f0, fmt in itertools.product(formats(), PF.SUBSAMPS):
        if not PF.valid(f0["layout"], f0["depth"], fmt):
            continue
        x = rng.integers(0, 256, (2, A.frame_bytes(w, h, fmt)), dtype=np.uint8)
        for f in paddings(f0, w, h, fmt):
            fb = PF.frame_bytes(f, w, h, fmt)
            before = rng.integers(0, 256, 2 * fb, dtype=np.uint8)
            buf = PO.export(x, f, w, h, fmt, fmt, 2, into=before.copy())
            assert np.array_equal(PF.convert(buf, f, w, h, fmt, 2), x), (f, fmt)
            # the bytes of the rows, and only those: over the inverted buffer exactly they come out the same
            other = PO.export(x, f, w, h, fmt, fmt, 2, into=~before)
            lay, _, _ = PF.plane_layout(f, w, h, fmt)
            assert (other == buf).sum() == 2 * sum(rb * nr for _, _, rb, nr in lay)
            assert np.array_equal(buf[other != buf], before[other != buf])
            if f["depth"] > 8:                           # every unused bit of a word is zero
                words = np.ascontiguousarray(PO.export(x, f0, w, h, fmt, fmt, 2)).view("<u2")
                used = (0xFF << 8) if f["msb"] else (0xFF << (f["depth"] - 8))
                assert not (words & ~np.uint16(used)).any()
            ncases += 1
    assert ncases >= 2 * 40


def test_validity_table(pkg):
    """every (stream subsampling, output subsampling, layout, depth): valid exactly where the pair is allowed and the layout is valid
    at the OUTPUT subsampling; the sizes agree; dsv1_export_clip refuses the others before it looks for a device"""
    L = pkg.lib()
    w, h = 35, 19
    src = np.zeros(A.frame_bytes(w, h, A.SUBSAMP_444), dtype=np.uint8)
    dst = np.zeros(8 * w * h + 4096, dtype=np.uint8)
    nvalid = ninvalid = 0
    for fmt, ofmt, f in itertools.product(PF.SUBSAMPS, PF.SUBSAMPS, formats()):
        pair = (ofmt == fmt or (fmt == A.SUBSAMP_444 and ofmt in (A.SUBSAMP_422, A.SUBSAMP_420)) or (fmt == A.SUBSAMP_422 and ofmt == A.SUBSAMP_420))
        lay_ok = (f["layout"] == PF.PLANAR or (f["layout"] in (PF.SEMI_UV, PF.SEMI_VU) and ofmt in (A.SUBSAMP_420, A.SUBSAMP_422))
                  or (f["layout"] in (PF.YUYV, PF.UYVY) and ofmt == A.SUBSAMP_422 and f["depth"] == 8))
        assert PO.allowed_pair(fmt, ofmt) == pair
        assert PO.valid(f, w, h, fmt, ofmt) == (pair and lay_ok), (fmt, ofmt, f)
        assert L.dsv1_pix_frame_bytes(C.byref(cpf(pkg, f)), w, h, ofmt) == PF.frame_bytes(f, w, h, ofmt)
        rc = L.dsv1_export_clip(NODEV, src.ctypes.data, w, h, fmt, 1, dst.ctypes.data, C.byref(cpf(pkg, f)), ofmt, 0)
        if pair and lay_ok:
            assert rc not in (0, DSVG_ERR_ARG), (fmt, ofmt, f)      # past the checks, to the device
            nvalid += 1
        else:
            assert rc == DSVG_ERR_ARG, (fmt, ofmt, f)
            ninvalid += 1
    assert nvalid > 60 and ninvalid > 150
    assert not dst.any()
    # upsampling, anything from 4:1:1, an unknown code
    nv12 = C.byref(cpf(pkg, PF.pf(PF.SEMI_UV)))
    plain = C.byref(cpf(pkg, PF.pf()))
    for fmt, ofmt in [(A.SUBSAMP_422, A.SUBSAMP_444), (A.SUBSAMP_420, A.SUBSAMP_422), (A.SUBSAMP_420, A.SUBSAMP_444), (A.SUBSAMP_411, A.SUBSAMP_420),
                      (A.SUBSAMP_411, A.SUBSAMP_422), (A.SUBSAMP_444, A.SUBSAMP_411), (A.SUBSAMP_444, 3), (3, 3)]:
        assert L.dsv1_export_clip(NODEV, src.ctypes.data, w, h, fmt, 1, dst.ctypes.data, plain, ofmt, 0) == DSVG_ERR_ARG, (fmt, ofmt)
    # bad pitches and strides are the format's, at the output subsampling
    for f in (PF.pf(PF.SEMI_UV, pitch=(w - 1, 0, 0)), PF.pf(PF.SEMI_UV, pitch=(0, 2 * ((w + 1) // 2) - 1, 0)), PF.pf(PF.SEMI_UV, frame_bytes=w * h),
              PF.pf(PF.PLANAR, 10, 2), PF.pf(PF.PLANAR, 9)):
        assert L.dsv1_export_clip(NODEV, src.ctypes.data, w, h, A.SUBSAMP_444, 1, dst.ctypes.data, C.byref(cpf(pkg, f)), A.SUBSAMP_420, 0) == DSVG_ERR_ARG, f
    # the argument errors
    s, d = src.ctypes.data, dst.ctypes.data
    for args in [(NODEV, None, w, h, A.SUBSAMP_420, 1, d, nv12, A.SUBSAMP_420, 0), (NODEV, s, w, h, A.SUBSAMP_420, 1, None, nv12, A.SUBSAMP_420, 0),
                 (NODEV, s, w, h, A.SUBSAMP_420, 1, d, None, A.SUBSAMP_420, 0), (NODEV, s, w, h, A.SUBSAMP_420, 0, d, nv12, A.SUBSAMP_420, 0),
                 (NODEV, s, 0, h, A.SUBSAMP_420, 1, d, nv12, A.SUBSAMP_420, 0), (-1, s, w, h, A.SUBSAMP_420, 1, d, nv12, A.SUBSAMP_420, 0)]:
        assert L.dsv1_export_clip(*args) == DSVG_ERR_ARG


def test_decbatch_entry_points_refuse_a_null_handle(pkg):
    L = pkg.lib()
    assert L.dsv1_decbatch_set_output_format(None, C.byref(cpf(pkg, PF.pf(PF.SEMI_UV))), A.SUBSAMP_420) == DSVG_ERR_ARG
    assert L.dsv1_decbatch_set_output_format(None, None, A.SUBSAMP_420) == DSVG_ERR_ARG
    assert L.dsv1_decbatch_out_frame_bytes(None) == 0
    with pytest.raises(ValueError):
        pkg.export_clip(np.zeros(100, dtype=np.uint8), 16, 16, A.SUBSAMP_420, cpf(pkg, PF.pf(PF.SEMI_UV)))
