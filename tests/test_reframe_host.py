"""Reframe and bar detection without a device (include/dsv1_api.h, Reframe): dsv1_reframe_valid and dsv1_bars_from_sums equal the numpy
statement tests/_reframe.py over tables with one case per rule; the model has the properties the header promises; the standalone
calls report a missing device and write nothing; every entry point refuses invalid input before it looks for a device."""
import ctypes as C

import numpy as np
import pytest

import _cabi as A
import _reframe as R

DSVG_ERR_ARG = -2
NO_DEVICE = 4096                                          # a device index no machine has


class Reframe(C.Structure):
    _fields_ = [("in_w", C.c_int), ("in_h", C.c_int), ("x", C.c_int), ("y", C.c_int), ("w", C.c_int), ("h", C.c_int), ("out_w", C.c_int),
                ("out_h", C.c_int), ("dst_x", C.c_int), ("dst_y", C.c_int), ("fill", C.c_uint8 * 3), ("reserved", C.c_uint8)]


class Meta(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("subsamp", C.c_int), ("fps_num", C.c_int), ("fps_den", C.c_int),
                ("aspect_num", C.c_int), ("aspect_den", C.c_int)]


def cs(r):
    return Reframe(r["in_w"], r["in_h"], r["x"], r["y"], r["w"], r["h"], r["out_w"], r["out_h"], r["dst_x"], r["dst_y"],
                   (C.c_uint8 * 3)(*r["fill"]), r["reserved"])


def prod():
    L = A.load_prod()
    L.dsv1_reframe_valid.argtypes = [C.POINTER(Reframe), C.c_int]
    L.dsv1_reframe_clip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(Reframe), C.c_int, C.c_int]
    L.dsv1_line_sums_clip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.dsv1_bars_from_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.dsv1_detect_bars_clip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    L.dsv1_batch_set_source_reframe.argtypes = [C.c_void_p, C.POINTER(Reframe)]
    L.dsv1_resladder_open_reframed.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(Reframe), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    return L


def test_the_struct_is_the_headers():
    assert C.sizeof(Reframe) == 44 and Reframe.fill.offset == 40 and Reframe.reserved.offset == 43


@pytest.mark.parametrize("name,r,expect", R.validity_table(), ids=[t[0] for t in R.validity_table()])
def test_validity(name, r, expect):
    L = prod()
    for fmt in R.FORMATS:
        want = expect[fmt] if isinstance(expect, dict) else expect
        assert R.valid(r, fmt) == want, "the model at 0x%x" % fmt
        assert bool(L.dsv1_reframe_valid(C.byref(cs(r)), fmt)) == want, "the library at 0x%x" % fmt
    for bad_fmt in (0x1, 0x6, 0x7, 0x9, -1, 0x15):
        assert not R.valid(r, bad_fmt) and L.dsv1_reframe_valid(C.byref(cs(r)), bad_fmt) == 0
    assert L.dsv1_reframe_valid(None, A.SUBSAMP_420) == 0


def test_the_table_violates_every_rule_once():
    names = [t[0] for t in R.validity_table()]
    assert len(set(names)) == len(names)
    false = [n for n, _, e in R.validity_table() if e is False]
    assert len(false) == 12 + 9 + 2 and sum(isinstance(e, dict) for _, _, e in R.validity_table()) == 6


def test_chroma_window_lies_inside_both_chroma_planes():
    """what the header derives from the rules, over every valid table entry and a sweep of odd sizes"""
    cases = [r for _, r, _ in R.validity_table()]
    cases += [R.rf(iw, 9, (x, 0, w, 5), (iw + 3, 9), (dx, 4)) for iw in (5, 8, 13) for x in (0, 4) for w in range(1, iw - x + 1) for dx in (0, 4) if dx + w <= iw + 3]
    n = 0
    for r in cases:
        for fmt in R.FORMATS:
            if not R.valid(r, fmt):
                continue
            hs, vs = A.hshift(fmt), A.vshift(fmt)
            icw, ich = A.chroma_dims(r["in_w"], r["in_h"], fmt)
            ocw, och = A.chroma_dims(r["out_w"], r["out_h"], fmt)
            W, H = A.rshift_up(r["w"], hs), A.rshift_up(r["h"], vs)
            assert (r["x"] >> hs) + W <= icw and (r["y"] >> vs) + H <= ich and (r["dst_x"] >> hs) + W <= ocw and (r["dst_y"] >> vs) + H <= och
            n += 1
    assert n > 200


# ---- bars ----------------------------------------------------------------------------------------------------------------------
def lib_bars(L, rows, cols, thresh, align):
    rows, cols = np.ascontiguousarray(rows, dtype=np.uint32), np.ascontiguousarray(cols, dtype=np.uint32)
    n, h, w = rows.shape[0], rows.shape[1], cols.shape[1]
    rect = (C.c_int * 4)(7, 7, 7, 7)
    rc = L.dsv1_bars_from_sums(rows.ctypes.data, cols.ctypes.data, w, h, n, thresh, align, rect)
    assert rc in (0, 1), rc
    if rc == 0:
        assert tuple(rect) == (0, 0, 0, 0)
        return None
    return tuple(rect)


def sums_of(w, h, n, rect, level=200, frames=None):
    """sums of n frames that are `level` inside rect (x, y, w, h) and 0 outside; frames: the frames that have content at all"""
    y = np.zeros((n, h, w), dtype=np.uint64)
    for t in (range(n) if frames is None else frames):
        y[t, rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = level
    return y.sum(axis=2).astype(np.uint32), y.sum(axis=1).astype(np.uint32)


BAR_CASES = [("none", (0, 0, 96, 64)), ("top", (0, 9, 96, 55)), ("bottom", (0, 0, 96, 51)), ("left", (13, 0, 83, 64)), ("right", (0, 0, 77, 64)),
             ("all four", (13, 9, 64, 42)), ("narrow column", (37, 0, 13, 64)), ("narrow row", (0, 21, 96, 9))]


@pytest.mark.parametrize("name,rect", BAR_CASES, ids=[c[0] for c in BAR_CASES])
def test_bars_every_side_and_align(name, rect):
    L = prod()
    rows, cols = sums_of(96, 64, 2, rect)
    found = set()
    for align in (1, 2, 4, 8, 16, 32, 64):
        want = R.bars_from_sums(rows, cols, 24, align)
        assert lib_bars(L, rows, cols, 24, align) == want, align
        found.add(want)
        if align == 1:
            assert want == rect
        elif want is not None:                           # rounded INWARD
            assert want[0] >= rect[0] and want[1] >= rect[1] and want[0] + want[2] <= rect[0] + rect[2] and want[1] + want[3] <= rect[1] + rect[3]
            assert all(v % align == 0 for v in want)
    if name in ("narrow column", "narrow row", "all four"):
        assert None in found                             # a rounding that leaves nothing


def test_bars_black_clip_one_frame_and_the_threshold():
    L = prod()
    w, h = 48, 32
    zr, zc = np.zeros((3, h), dtype=np.uint32), np.zeros((3, w), dtype=np.uint32)
    assert lib_bars(L, zr, zc, 0, 1) is None and R.bars_from_sums(zr, zc, 0, 1) is None               # all black
    # content in one frame only: the union over the frames
    rows, cols = sums_of(w, h, 3, (8, 4, 30, 20), frames=[1])
    assert lib_bars(L, rows, cols, 24, 2) == R.bars_from_sums(rows, cols, 24, 2) == (8, 4, 30, 20)
    # the union of different rectangles in different frames
    r0, c0 = sums_of(w, h, 1, (8, 4, 10, 10))
    r1, c1 = sums_of(w, h, 1, (20, 16, 20, 12))
    rows, cols = np.concatenate([r0, r1]), np.concatenate([c0, c1])
    assert lib_bars(L, rows, cols, 24, 1) == R.bars_from_sums(rows, cols, 24, 1) == (8, 4, 32, 24)
    # the boundary: a sum EQUAL to thresh * length is not content, one more is
    for thresh in (0, 1, 24, 254):
        rows = np.full((1, h), thresh * w, dtype=np.uint32)
        cols = np.full((1, w), thresh * h, dtype=np.uint32)
        assert lib_bars(L, rows, cols, thresh, 1) is None and R.bars_from_sums(rows, cols, thresh, 1) is None
        rows[0, 5:9] += 1
        assert lib_bars(L, rows, cols, thresh, 1) is None                                               # rows alone are no rectangle
        cols[0, 7:20] += 1
        assert lib_bars(L, rows, cols, thresh, 1) == R.bars_from_sums(rows, cols, thresh, 1) == (7, 5, 13, 4)
    # a column's mean includes the rows of horizontal bars (the header's known consequence): dim content inside a letterbox is lost
    rows, cols = sums_of(w, h, 1, (0, 12, w, 8), level=40)
    assert (cols[0] == 40 * 8).all() and 40 * 8 <= 24 * h and lib_bars(L, rows, cols, 24, 1) is None


def test_bars_arguments():
    L = prod()
    rows, cols = sums_of(16, 16, 1, (0, 0, 16, 16))
    rect = (C.c_int * 4)(7, 7, 7, 7)
    for thresh, align in ((-1, 2), (255, 2), (24, 0), (24, 3), (24, 128), (24, -2), (24, 6)):
        assert not R.bars_ok(thresh, align)
        assert L.dsv1_bars_from_sums(rows.ctypes.data, cols.ctypes.data, 16, 16, 1, thresh, align, rect) == DSVG_ERR_ARG
        assert L.dsv1_detect_bars_clip(0, rows.ctypes.data, 16, 16, A.SUBSAMP_420, 1, thresh, align, rect, 0) == DSVG_ERR_ARG
    for thresh, align in ((0, 1), (254, 64)):
        assert R.bars_ok(thresh, align) and L.dsv1_bars_from_sums(rows.ctypes.data, cols.ctypes.data, 16, 16, 1, thresh, align, rect) in (0, 1)
    assert L.dsv1_bars_from_sums(None, cols.ctypes.data, 16, 16, 1, 24, 2, rect) == DSVG_ERR_ARG
    assert L.dsv1_bars_from_sums(rows.ctypes.data, cols.ctypes.data, 0, 16, 1, 24, 2, rect) == DSVG_ERR_ARG
    assert L.dsv1_bars_from_sums(rows.ctypes.data, cols.ctypes.data, 16, 16, 0, 24, 2, rect) == DSVG_ERR_ARG


# ---- the model -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_model_crop_then_pad_back_and_identity(fmt):
    w, h = 70, 50
    clip = R.noise(2, w, h, fmt, 0x5EF)
    ident = R.rf(w, h, (0, 0, w, h), (w, h))
    assert np.array_equal(R.reframe_clip(clip, ident, fmt), clip)
    win = (8, 4, 51, 33)
    crop = R.rf(w, h, win, (51, 33))
    back = R.rf(51, 33, (0, 0, 51, 33), (w, h), (8, 4), (1, 2, 3))
    cut = R.reframe_clip(clip, crop, fmt)
    assert cut.shape == (2, A.frame_bytes(51, 33, fmt))
    padded = R.reframe_clip(cut, back, fmt)
    direct = R.reframe_clip(clip, R.rf(w, h, win, (w, h), (8, 4), (1, 2, 3)), fmt)
    assert np.array_equal(padded, direct)
    for p, (a, b) in enumerate(zip(R.planes(padded[1], w, h, fmt), R.planes(clip[1], w, h, fmt))):
        hs, vs = (A.hshift(fmt), A.vshift(fmt)) if p else (0, 0)
        X, Y, W, H = 8 >> hs, 4 >> vs, A.rshift_up(51, hs), A.rshift_up(33, vs)
        assert np.array_equal(a[Y:Y + H, X:X + W], b[Y:Y + H, X:X + W])      # the window is restored
        mask = np.ones(a.shape, dtype=bool)
        mask[Y:Y + H, X:X + W] = False
        assert (a[mask] == p + 1).all()                                        # and everything else is the fill
    rows, cols = R.line_sums(clip, w, h, fmt)
    assert rows.shape == (2, h) and cols.shape == (2, w) and int(rows[1].sum()) == int(cols[1].sum()) == int(clip[1, :w * h].astype(np.int64).sum())


def test_model_gpu_cases_are_valid_and_reach_every_subsampling():
    seen = set()
    for name, r, n in R.gpu_cases():
        fmts = R.formats_of(r)
        assert fmts, name
        seen.update(fmts)
    assert seen == set(R.FORMATS)
    odd = R.gpu_cases()[0][1]
    assert R.formats_of(odd) == [A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420]      # (x = 6 is no multiple of 4: 4:1:1 has its own case)
    # the source is off the destination by (x - dst_x) + row * (in_w - out_w): another value mod 4 from row to row, odd ones included in chroma
    assert odd["in_w"] % 16 and odd["w"] % 2 and (odd["in_w"] - odd["out_w"]) % 4 and ((odd["in_w"] >> 1) - (odd["out_w"] >> 1)) % 2


# ---- no device -----------------------------------------------------------------------------------------------------------------
def test_standalone_calls_report_a_missing_device_and_write_nothing():
    L = prod()
    fmt = A.SUBSAMP_420
    r = R.rf(16, 16, (0, 0, 16, 16), (32, 32), (8, 8))
    src = R.noise(1, 16, 16, fmt, 1)
    dst = np.full(A.frame_bytes(32, 32, fmt), 0xA5, dtype=np.uint8)
    rc = L.dsv1_reframe_clip(NO_DEVICE, src.ctypes.data, 1, dst.ctypes.data, C.byref(cs(r)), fmt, 0)
    assert rc < 0 and rc != DSVG_ERR_ARG and (dst == 0xA5).all()
    rows, cols = np.full(16, 0xA5A5A5A5, dtype=np.uint32), np.full(16, 0xA5A5A5A5, dtype=np.uint32)
    rc = L.dsv1_line_sums_clip(NO_DEVICE, src.ctypes.data, 16, 16, fmt, 1, rows.ctypes.data, cols.ctypes.data, 0)
    assert rc < 0 and rc != DSVG_ERR_ARG and (rows == 0xA5A5A5A5).all() and (cols == 0xA5A5A5A5).all()
    rect = (C.c_int * 4)(7, 7, 7, 7)
    rc = L.dsv1_detect_bars_clip(NO_DEVICE, src.ctypes.data, 16, 16, fmt, 1, 24, 2, rect, 0)
    assert rc < 0 and rc != DSVG_ERR_ARG and tuple(rect) == (0, 0, 0, 0)


def test_invalid_input_is_refused_before_a_device_is_looked_for():
    L = prod()
    fmt = A.SUBSAMP_420
    buf = np.full(8192, 0xA5, dtype=np.uint8)
    ok = R.rf(16, 16, (0, 0, 16, 16), (32, 32), (8, 8))
    p = buf.ctypes.data
    for dev in (0, NO_DEVICE):
        for bad in (dict(ok, x=1), dict(ok, w=17), dict(ok, reserved=3), dict(ok, out_w=0)):
            assert L.dsv1_reframe_clip(dev, p, 1, p, C.byref(cs(bad)), fmt, 0) == DSVG_ERR_ARG
        assert L.dsv1_reframe_clip(dev, p, 1, p, None, fmt, 0) == DSVG_ERR_ARG
        assert L.dsv1_reframe_clip(dev, p, 0, p, C.byref(cs(ok)), fmt, 0) == DSVG_ERR_ARG
        assert L.dsv1_reframe_clip(dev, None, 1, p, C.byref(cs(ok)), fmt, 0) == DSVG_ERR_ARG
        assert L.dsv1_reframe_clip(dev, p, 1, None, C.byref(cs(ok)), fmt, 0) == DSVG_ERR_ARG
        assert L.dsv1_reframe_clip(dev, p, 1, p, C.byref(cs(ok)), 0x7, 0) == DSVG_ERR_ARG
        assert L.dsv1_reframe_clip(-1, p, 1, p, C.byref(cs(ok)), fmt, 0) == DSVG_ERR_ARG
        for w, h, f, n in ((0, 16, fmt, 1), (16, -1, fmt, 1), (16, 16, 0x7, 1), (16, 16, fmt, 0)):
            assert L.dsv1_line_sums_clip(dev, p, w, h, f, n, p, p, 0) == DSVG_ERR_ARG
            assert L.dsv1_detect_bars_clip(dev, p, w, h, f, n, 24, 2, (C.c_int * 4)(), 0) == DSVG_ERR_ARG
        assert L.dsv1_line_sums_clip(dev, None, 16, 16, fmt, 1, p, p, 0) == DSVG_ERR_ARG
        assert L.dsv1_line_sums_clip(dev, p, 16, 16, fmt, 1, None, p, 0) == DSVG_ERR_ARG
        assert L.dsv1_line_sums_clip(dev, p, 16, 16, fmt, 1, p, None, 0) == DSVG_ERR_ARG
        assert L.dsv1_detect_bars_clip(dev, p, 16, 16, fmt, 1, 24, 2, None, 0) == DSVG_ERR_ARG
    assert (buf == 0xA5).all()
    assert L.dsv1_batch_set_source_reframe(None, C.byref(cs(ok))) == DSVG_ERR_ARG
    # the resolution ladder's open: src is not the reframe's input; an invalid reframe; both a format and an RGB format
    out = C.c_void_p(None)
    meta = Meta(16, 16, fmt, 30, 1, 1, 1)
    other = Meta(32, 32, fmt, 30, 1, 1, 1)
    dummy = buf.ctypes.data
    assert L.dsv1_resladder_open_reframed(C.byref(out), C.byref(other), C.byref(cs(ok)), None, fmt, None, dummy, 1, NO_DEVICE, 1, 1, 1) == DSVG_ERR_ARG
    assert L.dsv1_resladder_open_reframed(C.byref(out), C.byref(meta), C.byref(cs(dict(ok, x=1))), None, fmt, None, dummy, 1, NO_DEVICE, 1, 1, 1) == DSVG_ERR_ARG
    assert L.dsv1_resladder_open_reframed(C.byref(out), C.byref(meta), C.byref(cs(ok)), dummy, fmt, dummy, dummy, 1, NO_DEVICE, 1, 1, 1) == DSVG_ERR_ARG
    assert L.dsv1_resladder_open_reframed(C.byref(out), None, C.byref(cs(ok)), None, fmt, None, dummy, 1, NO_DEVICE, 1, 1, 1) == DSVG_ERR_ARG
    assert out.value is None
