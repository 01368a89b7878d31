"""The eight orientations without a device (include/dsv1_api.h, Orientation): dsv1_orient_valid, _dims, _compose, _inverse, _from_exif and
_from_matrix equal the numpy statement tests/_orient.py; the statement itself is numpy's rot90 where the header says so; the standalone
call refuses invalid input before it looks for a device."""
import ctypes as C

import numpy as np

import _cabi as A
import _orient as O

DSVG_ERR_ARG = -2
NO_DEVICE = 4096                                          # a device index no machine has


def prod():
    L = A.load_prod()
    L.dsv1_orient_valid.argtypes = [C.c_int, C.c_int]
    L.dsv1_orient_dims.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.dsv1_orient_compose.argtypes = [C.c_int, C.c_int]
    L.dsv1_orient_inverse.argtypes = [C.c_int]
    L.dsv1_orient_from_exif.argtypes = [C.c_int]
    L.dsv1_orient_from_matrix.argtypes = [C.POINTER(C.c_int32)]
    L.dsv1_orient_clip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    return L


def from_matrix(L, m):
    return L.dsv1_orient_from_matrix((C.c_int32 * 9)(*m))


def test_constants_are_the_headers():
    hdr = open(A.ROOT + "/include/dsv1_api.h").read()
    enum = hdr[hdr.index("enum { DSV1_ORIENT_NONE"):]
    enum = enum[:enum.index("}")]
    names = [x.strip() for x in enum[enum.index("{") + 1:].replace("\n", " ").split(",")]
    assert names == ["DSV1_ORIENT_" + n.upper() for n in O.NAMES]


def test_valid_and_dims():
    L = prod()
    for code in range(-1, 9):
        for fmt in O.FORMATS + (0x1, 0x6, 0x15, -1):
            assert bool(L.dsv1_orient_valid(code, fmt)) == O.valid(code, fmt), (code, hex(fmt))
        for w, h in ((5, 7), (1, 1), (1920, 1080)):
            ow, oh = C.c_int(-7), C.c_int(-7)
            rc = L.dsv1_orient_dims(code, w, h, C.byref(ow), C.byref(oh))
            want = O.dims(code, w, h)
            assert (rc == 0 and (ow.value, oh.value) == want) if want else rc == DSVG_ERR_ARG, (code, w, h)
    # transposing needs equal chroma shifts: 4:4:4 and 4:2:0 only
    assert [f for f in O.FORMATS if O.valid(O.ROT90, f)] == [A.SUBSAMP_444, A.SUBSAMP_420]
    ow, oh = C.c_int(0), C.c_int(0)
    assert L.dsv1_orient_dims(O.ROT90, 0, 4, C.byref(ow), C.byref(oh)) == DSVG_ERR_ARG
    assert L.dsv1_orient_dims(O.ROT90, 4, 0, C.byref(ow), C.byref(oh)) == DSVG_ERR_ARG
    assert L.dsv1_orient_dims(O.ROT90, 4, 4, None, C.byref(oh)) == DSVG_ERR_ARG


def test_compose():
    L = prod()
    probe = np.arange(35).reshape(5, 7)
    for a in range(8):
        for b in range(8):
            c = L.dsv1_orient_compose(a, b)
            assert c == O.compose(a, b), (a, b)
            assert np.array_equal(O.plane(O.plane(probe, a), b), O.plane(probe, c)), (a, b)
        inv = L.dsv1_orient_inverse(a)
        assert inv == O.inverse(a) and L.dsv1_orient_compose(a, inv) == O.NONE and L.dsv1_orient_compose(inv, a) == O.NONE
    c = O.NONE
    for k in range(4):
        assert (c == O.NONE) == (k == 0)
        c = L.dsv1_orient_compose(c, O.ROT90)
    assert c == O.NONE
    assert L.dsv1_orient_compose(O.ROT90, O.ROT90) == O.ROT180 and L.dsv1_orient_compose(O.ROT90, O.ROT270) == O.NONE
    for bad in (-1, 8):
        assert L.dsv1_orient_compose(bad, 0) == DSVG_ERR_ARG and L.dsv1_orient_compose(0, bad) == DSVG_ERR_ARG
        assert L.dsv1_orient_inverse(bad) == DSVG_ERR_ARG


def test_from_exif():
    L = prod()
    assert [L.dsv1_orient_from_exif(t) for t in range(1, 9)] == [0, 1, 3, 2, 4, 5, 7, 6]
    for t in range(0, 10):
        assert L.dsv1_orient_from_exif(t) == O.EXIF.get(t, DSVG_ERR_ARG)
    assert L.dsv1_orient_from_exif(-1) == DSVG_ERR_ARG


def test_from_matrix():
    L = prod()
    probe = np.arange(35).reshape(5, 7)
    for code, abcd in O.MATRICES.items():
        m = O.matrix(*abcd)
        assert from_matrix(L, m) == code, O.NAMES[code]
        assert np.array_equal(O.place_by_matrix(probe, m), O.plane(probe, code)), O.NAMES[code]
        # translation and the third column are ignored
        assert from_matrix(L, O.matrix(*abcd, tx=1080 << 16, ty=-(7 << 16), u=5, v=-3, w=0)) == code
    one = 65536
    r = 46341                                             # cos 45 = sin 45 in 16.16
    refused = {"45 degrees": [r, r, 0, -r, r, 0, 0, 0, 1 << 30], "scaled": [2 * one, 0, 0, 0, one, 0, 0, 0, 1 << 30],
               "scaled rotation": [0, 2 * one, 0, -one, 0, 0, 0, 0, 1 << 30], "sheared": [one, 0, 0, one, one, 0, 0, 0, 1 << 30],
               "all zero": [0] * 9, "a and b": [one, one, 0, 0, 0, 0, 0, 0, 1 << 30], "a and b and d": [one, one, 0, 0, one, 0, 0, 0, 1 << 30],
               "half": [one // 2, 0, 0, 0, one, 0, 0, 0, 1 << 30], "c and d": [0, 0, 0, one, one, 0, 0, 0, 1 << 30]}
    for name, m in refused.items():
        assert from_matrix(L, m) == DSVG_ERR_ARG, name
    assert L.dsv1_orient_from_matrix(None) == DSVG_ERR_ARG


def test_the_definition_is_numpys():
    rng = np.random.default_rng(7)
    for shape in ((5, 7), (1, 9), (64, 3)):
        i = rng.integers(0, 256, size=shape, dtype=np.uint8)
        assert np.array_equal(O.plane(i, O.NONE), i)
        assert np.array_equal(O.plane(i, O.HFLIP), i[:, ::-1]) and np.array_equal(O.plane(i, O.VFLIP), i[::-1])
        assert np.array_equal(O.plane(i, O.ROT180), np.rot90(i, 2)) and np.array_equal(O.plane(i, O.TRANSPOSE), i.T)
        assert np.array_equal(O.plane(i, O.ROT90), np.rot90(i, -1))
        assert np.array_equal(O.plane(i, O.ROT270), np.rot90(i, 1))
        assert np.array_equal(O.plane(i, O.TRANSVERSE), np.rot90(i, 2).T)
        # the bit set: transpose first, then mirror the columns, then the rows
        for code in range(8):
            t = i.T if code & 4 else i
            t = t[:, ::-1] if code & 1 else t
            t = t[::-1] if code & 2 else t
            assert np.array_equal(O.plane(i, code), t), code


def test_a_420_frame_of_7x5_turns_into_a_frame_of_5x7():
    """the transposed chroma plane IS the chroma plane of the output geometry, odd sizes included"""
    fmt, w, h = A.SUBSAMP_420, 7, 5
    clip = O.noise(2, w, h, fmt, 3)
    assert A.chroma_dims(w, h, fmt) == (4, 3) and A.chroma_dims(h, w, fmt) == (3, 4)
    for code in (O.TRANSPOSE, O.ROT90, O.ROT270, O.TRANSVERSE):
        out = O.orient_clip(clip, w, h, fmt, code)
        assert out.shape == clip.shape
        for t in range(2):
            for i, o in zip(O.planes(clip[t], w, h, fmt), O.planes(out[t], h, w, fmt)):
                assert o.shape == i.shape[::-1] and np.array_equal(o, O.plane(i, code))
        assert np.array_equal(O.planes(out[0], h, w, fmt)[1], {O.TRANSPOSE: lambda p: p.T, O.ROT90: lambda p: np.rot90(p, -1),
                                                                O.ROT270: lambda p: np.rot90(p, 1), O.TRANSVERSE: lambda p: np.rot90(p, 2).T}[code](
            O.planes(clip[0], w, h, fmt)[1]))
        back = O.orient_clip(out, h, w, fmt, O.inverse(code))
        assert np.array_equal(back, clip)
    # every size: the frame keeps its length under every valid code
    for fmt in O.FORMATS:
        for w, h in ((1, 1), (3, 5), (8, 6), (9, 2)):
            for code in range(8):
                if O.valid(code, fmt):
                    assert A.frame_bytes(*O.dims(code, w, h), fmt) == A.frame_bytes(w, h, fmt)


def test_orient_clip_refuses_before_it_looks_for_a_device():
    L = prod()
    fmt, w, h = A.SUBSAMP_420, 8, 6
    src = O.noise(1, w, h, fmt, 1)
    dst = np.full_like(src, 0x5A)
    call = lambda **k: L.dsv1_orient_clip(k.get("dev", NO_DEVICE), k.get("src", src.ctypes.data), k.get("w", w), k.get("h", h), k.get("fmt", fmt),
                                          k.get("n", 1), k.get("dst", dst.ctypes.data), k.get("orient", O.ROT90), 0)
    for bad in (dict(src=None), dict(dst=None), dict(n=0), dict(n=-1), dict(w=0), dict(h=0), dict(orient=-1), dict(orient=8), dict(dev=-1),
                dict(fmt=A.SUBSAMP_422), dict(fmt=A.SUBSAMP_411), dict(fmt=0x7)):
        assert call(**bad) == DSVG_ERR_ARG, bad
    rc = call()
    assert rc < 0 and rc != DSVG_ERR_ARG                  # valid arguments: only now is the device missed
    assert (dst == 0x5A).all()
