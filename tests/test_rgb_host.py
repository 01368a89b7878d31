"""RGB on the host (no GPU): the library's tables against their derivation in exact rationals and against the issue's literals;
the numpy statement tests/_rgb.py against round-half-up real arithmetic over all 2^24 triples of each (matrix, range) pair, in both
directions; the clamp that binds; the validity table, decided before any device is looked at; import at a subsampling equals the
halved 4:4:4 import."""
import ctypes as C
import importlib
import itertools
import math
from fractions import Fraction as Fr

import numpy as np
import pytest

import _cabi as A
import _pixout as PO
import _rgb as RG

DSVG_ERR_ARG = -2
NODEV = 1 << 20          # a device number no machine has: a call that passes the checks fails there, not with DSVG_ERR_ARG
PAIRS = list(itertools.product(RG.MATRICES, (0, 1)))

# matrix, range -> Y row, Cb row, Cr row, (IY, RV, GU, GV, BU): the table of the definition
LITERALS = {
    (RG.BT601, 0): ([16829, 33039, 6416], [-9714, -19070, 28784], [28784, -24103, -4681], [19077, 26149, -6419, -13320, 33050]),
    (RG.BT601, 1): ([19595, 38470, 7471], [-11058, -21710, 32768], [32768, -27439, -5329], [16384, 22970, -5638, -11700, 29032]),
    (RG.BT709, 0): ([11966, 40254, 4064], [-6596, -22188, 28784], [28784, -26145, -2639], [19077, 29372, -3494, -8731, 34610]),
    (RG.BT709, 1): ([13933, 46871, 4732], [-7509, -25259, 32768], [32768, -29763, -3005], [16384, 25802, -3069, -7670, 30402]),
    (RG.BT2020, 0): ([14786, 38160, 3338], [-8038, -20746, 28784], [28784, -26469, -2315], [19077, 27503, -3069, -10657, 35091]),
    (RG.BT2020, 1): ([17216, 44434, 3886], [-9151, -23617, 32768], [32768, -30133, -2635], [16384, 24160, -2696, -9361, 30825]),
}


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("digital-subband-video-1_amd")


def crf(pkg, f):
    return pkg.RgbFormat(f["order"], f["matrix"], f["full"], f["upsample"], f["pitch"], f["frame_bytes"])


@pytest.mark.parametrize("matrix,full", PAIRS)
def test_tables_equal_the_derivation_and_the_literals(pkg, matrix, full):
    fwd, inv = pkg.rgb_tables(matrix, full)
    dfwd, dinv = RG.tables(matrix, full)
    assert fwd.tolist() == dfwd and inv.tolist() == dinv
    y, cb, cr, iv = LITERALS[(matrix, full)]
    assert dfwd == [y, cb, cr] and dinv == iv
    sy, sc, _ = RG.ranges(full)
    assert sum(dfwd[0]) == RG.r(65536 * sy) and sum(dfwd[1]) == 0 and sum(dfwd[2]) == 0
    assert dfwd[1][2] == dfwd[2][0] == RG.r(65536 * sc / 2)


def test_tables_refuse_unknown_arguments(pkg):
    L = pkg.lib()
    fwd, inv = (C.c_int32 * 9)(), (C.c_int32 * 5)()
    for m, f in [(-1, 0), (3, 0), (0, 2), (0, -1)]:
        assert L.dsv1_rgb_tables(m, f, fwd, inv) == DSVG_ERR_ARG
        with pytest.raises(ValueError):
            pkg.rgb_tables(m, f)


def _round_half_up(num, den):
    """numpy int64 numerators over one positive python-int denominator"""
    return (2 * num + den) // (2 * den)


def _lin(coefs, xs):
    """sum of Fraction coefficients times int64 arrays as (numerator array, common denominator)"""
    den = 1
    for c in coefs:
        den = den * c.denominator // math.gcd(den, c.denominator)
    den = int(den)
    num = sum(int(c.numerator * (den // c.denominator)) * x for c, x in zip(coefs, xs))
    return num, den


@pytest.mark.parametrize("matrix,full", PAIRS)
def test_forward_is_within_one_of_real_arithmetic_over_all_triples(matrix, full):
    """Y = oy + sy (Kr R + Kg G + Kb B), Cb = 128 + sc (B - Y') / (2 (1 - Kb)), Cr = 128 + sc (R - Y') / (2 (1 - Kr)), rounded half up
    and clamped: the integer tables differ by at most 1 (each coefficient is off by at most half a unit of 2^-16, times 255, three
    times over: under one unit before the rounding)"""
    kr, kb = RG.K[matrix]
    kg = 1 - kr - kb
    sy, sc, oy = RG.ranges(full)
    rows = [([sy * kr, sy * kg, sy * kb], oy),
            ([-sc * kr / (2 * (1 - kb)), -sc * kg / (2 * (1 - kb)), sc / 2], 128),
            ([sc / 2, -sc * kg / (2 * (1 - kr)), -sc * kb / (2 * (1 - kr))], 128)]
    G, B = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    worst, differ = 0, 0
    for r0 in range(0, 256, 16):
        R = np.repeat(np.arange(r0, r0 + 16, dtype=np.int64), 65536).reshape(16, 256, 256)
        got = RG.to_ycc(R, G[None], B[None], matrix, full)
        for (coefs, off), g in zip(rows, got):
            num, den = _lin(coefs, (R, G[None], B[None]))
            want = np.clip(_round_half_up(num, den) + off, 0, 255)
            d = np.abs(g - want)
            worst = max(worst, int(d.max()))
            differ += int((d != 0).sum())
    print("matrix %d full %d: forward worst %d, %d of %d components differ" % (matrix, full, worst, differ, 3 << 24))
    assert worst <= 1


@pytest.mark.parametrize("matrix,full", PAIRS)
def test_inverse_is_within_one_of_real_arithmetic_over_all_triples(matrix, full):
    """R = y / sy + 2 (1 - Kr) v / sc, G = y / sy - (2 (1 - Kb) Kb u + 2 (1 - Kr) Kr v) / (Kg sc), B = y / sy + 2 (1 - Kb) u / sc with
    y = Y - oy, u = Cb - 128, v = Cr - 128, rounded half up and clamped"""
    kr, kb = RG.K[matrix]
    kg = 1 - kr - kb
    sy, sc, oy = RG.ranges(full)
    rows = [[1 / sy, Fr(0), 2 * (1 - kr) / sc], [1 / sy, -2 * (1 - kb) * kb / (kg * sc), -2 * (1 - kr) * kr / (kg * sc)], [1 / sy, 2 * (1 - kb) / sc, Fr(0)]]
    U, V = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    worst, differ = 0, 0
    for y0 in range(0, 256, 16):
        Y = np.repeat(np.arange(y0, y0 + 16, dtype=np.int64), 65536).reshape(16, 256, 256)
        got = RG.to_rgb(Y, U[None], V[None], matrix, full)
        for coefs, g in zip(rows, got):
            num, den = _lin(coefs, (Y - oy, U[None] - 128, V[None] - 128))
            want = np.clip(_round_half_up(num, den), 0, 255)
            d = np.abs(g - want)
            worst = max(worst, int(d.max()))
            differ += int((d != 0).sum())
    print("matrix %d full %d: inverse worst %d, %d of %d components differ" % (matrix, full, worst, differ, 3 << 24))
    assert worst <= 1


@pytest.mark.parametrize("matrix", RG.MATRICES)
def test_full_range_pure_blue_and_red_hit_the_clamp(matrix):
    one = np.array([255]), np.array([0])
    _, cb, _ = RG.to_ycc(one[1], one[1], one[0], matrix, 1, clamp=False)
    _, _, cr = RG.to_ycc(one[0], one[1], one[1], matrix, 1, clamp=False)
    assert cb[0] == 256 and cr[0] == 256
    assert RG.to_ycc(one[1], one[1], one[0], matrix, 1)[1][0] == 255 and RG.to_ycc(one[0], one[1], one[1], matrix, 1)[2][0] == 255


def invalid_formats(w, h):
    good = RG.rf()
    yield dict(good, order=-1)
    yield dict(good, order=8)
    yield dict(good, matrix=3)
    yield dict(good, matrix=-1)
    yield dict(good, full=2)
    yield dict(good, full=-1)
    yield dict(good, upsample=2)
    yield dict(good, upsample=-1)
    yield dict(good, pitch=(3 * w - 1, 0, 0))
    yield dict(good, pitch=(-1, 0, 0))
    yield dict(good, order=RG.BGRA, pitch=(4 * w - 1, 0, 0))
    yield dict(good, order=RG.PLANAR_GBR, pitch=(0, w - 1, 0))
    yield dict(good, order=RG.PLANAR_RGB, pitch=(0, 0, w - 1))
    yield dict(good, frame_bytes=3 * w * h - 1)
    yield dict(good, order=RG.PLANAR_RGB, pitch=(w + 4, 0, 0), frame_bytes=3 * w * h + 4 * h - 1)


def test_frame_bytes_follows_the_layout(pkg):
    for (w, h), order in itertools.product([(352, 288), (35, 19), (1, 1)], RG.ORDERS):
        bpp = 3 if order <= RG.BGR24 else 4 if order <= RG.ABGR else 1
        f = RG.rf(order)
        assert pkg.rgb_frame_bytes(crf(pkg, f), w, h) == RG.frame_bytes(f, w, h) == (3 * w * h if bpp == 1 else bpp * w * h)
        g = RG.rf(order, pitch=(bpp * w + 5, w + 3, w + 16), frame_bytes=0)
        assert pkg.rgb_frame_bytes(crf(pkg, g), w, h) == RG.frame_bytes(g, w, h)
        g = dict(g, frame_bytes=RG.frame_bytes(g, w, h) + 37)
        assert pkg.rgb_frame_bytes(crf(pkg, g), w, h) == RG.frame_bytes(g, w, h)


def test_every_invalid_combination_is_refused_with_no_device(pkg):
    L = pkg.lib()
    w, h = 36, 20
    src = np.zeros(4 * w * h * 2, dtype=np.uint8)
    dst = np.zeros(4 * w * h * 2, dtype=np.uint8)
    for f in invalid_formats(w, h):
        assert RG.layout(f, w, h) is None, f
        c = crf(pkg, f)
        assert L.dsv1_rgb_frame_bytes(C.byref(c), w, h) == 0, f
        with pytest.raises(ValueError):
            pkg.rgb_frame_bytes(c, w, h)
        assert L.dsv1_rgb_import_clip(NODEV, src.ctypes.data, C.byref(c), w, h, A.SUBSAMP_420, 1, dst.ctypes.data, 0) == DSVG_ERR_ARG, f
        assert L.dsv1_rgb_export_clip(NODEV, src.ctypes.data, w, h, A.SUBSAMP_420, 1, dst.ctypes.data, C.byref(c), 0) == DSVG_ERR_ARG, f
    good = crf(pkg, RG.rf())
    for bad_w, bad_h in [(0, h), (w, 0), (-1, h)]:
        assert L.dsv1_rgb_frame_bytes(C.byref(good), bad_w, bad_h) == 0
    assert L.dsv1_rgb_frame_bytes(None, w, h) == 0
    # 4:1:1 and unknown subsamplings, both ways; null pointers and n < 1
    for sub in (A.SUBSAMP_411, 0x1, 0x6, 0xF):
        assert L.dsv1_rgb_import_clip(NODEV, src.ctypes.data, C.byref(good), w, h, sub, 1, dst.ctypes.data, 0) == DSVG_ERR_ARG
        assert L.dsv1_rgb_export_clip(NODEV, src.ctypes.data, w, h, sub, 1, dst.ctypes.data, C.byref(good), 0) == DSVG_ERR_ARG
    assert L.dsv1_rgb_import_clip(NODEV, None, C.byref(good), w, h, A.SUBSAMP_420, 1, dst.ctypes.data, 0) == DSVG_ERR_ARG
    assert L.dsv1_rgb_import_clip(NODEV, src.ctypes.data, None, w, h, A.SUBSAMP_420, 1, dst.ctypes.data, 0) == DSVG_ERR_ARG
    assert L.dsv1_rgb_import_clip(NODEV, src.ctypes.data, C.byref(good), w, h, A.SUBSAMP_420, 0, dst.ctypes.data, 0) == DSVG_ERR_ARG
    assert L.dsv1_rgb_export_clip(NODEV, src.ctypes.data, w, h, A.SUBSAMP_420, 1, None, C.byref(good), 0) == DSVG_ERR_ARG
    # a valid call gets past the checks and fails at the device instead
    assert L.dsv1_rgb_import_clip(NODEV, src.ctypes.data, C.byref(good), w, h, A.SUBSAMP_420, 1, dst.ctypes.data, 0) not in (0, DSVG_ERR_ARG)
    assert L.dsv1_rgb_export_clip(NODEV, src.ctypes.data, w, h, A.SUBSAMP_420, 1, dst.ctypes.data, C.byref(good), 0) not in (0, DSVG_ERR_ARG)
    assert not dst.any()
    # setters and the opener refuse a NULL handle / format before anything else
    assert L.dsv1_batch_set_source_rgb(None, C.byref(good)) == DSVG_ERR_ARG
    assert L.dsv1_decbatch_set_output_rgb(None, C.byref(good)) == DSVG_ERR_ARG
    hnd = C.c_void_p(None)
    m = pkg.Meta()
    m.width, m.height, m.subsamp = 64, 64, A.SUBSAMP_420
    cfgs = (pkg.Encoder * 1)(pkg.make_encoder_cfg(64, 64, A.SUBSAMP_420))
    rung = (pkg.ResRung * 1)(pkg.ResRung(64, 64, 1, cfgs))
    assert L.dsv1_resladder_open_rgb(C.byref(hnd), C.byref(m), None, rung, 1, NODEV, 1, 1, 1) == DSVG_ERR_ARG and not hnd.value
    bad = crf(pkg, RG.rf(matrix=7))
    assert L.dsv1_resladder_open_rgb(C.byref(hnd), C.byref(m), C.byref(bad), rung, 1, NODEV, 1, 1, 1) == DSVG_ERR_ARG and not hnd.value
    m.subsamp = A.SUBSAMP_411
    assert L.dsv1_resladder_open_rgb(C.byref(hnd), C.byref(m), C.byref(good), rung, 1, NODEV, 1, 1, 1) == DSVG_ERR_ARG and not hnd.value


@pytest.mark.parametrize("w,h", [(36, 20), (35, 19), (1, 1), (2, 5)])
def test_import_at_a_subsampling_is_the_halved_444_import(w, h):
    rng = np.random.default_rng(w * h)
    for k, (order, (matrix, full)) in enumerate(itertools.product((RG.RGB24, RG.ABGR, RG.PLANAR_GBR), PAIRS)):
        f = RG.rf(order, matrix, full, pitch=(4 * w + 7, w + 1, w + 2) if k % 2 else (0, 0, 0))
        n = 2
        R, G, B = (rng.integers(0, 256, (n, h, w), dtype=np.uint8) for _ in range(3))
        R[0, 0, 0], G[0, 0, 0], B[0, 0, 0] = 0, 0, 255
        R[0, -1, -1], G[0, -1, -1], B[0, -1, -1] = 255, 0, 0
        buf = RG.pack(R, G, B, f, w, h, rng)
        got = RG.unpack(buf, f, w, h, n)
        assert all(np.array_equal(a, b) for a, b in zip(got, (R, G, B)))
        full444 = RG.import_(buf, f, w, h, A.SUBSAMP_444, n)
        for sub in RG.SUBSAMPS:
            assert np.array_equal(RG.import_(buf, f, w, h, sub, n), PO.planar_at(full444, w, h, A.SUBSAMP_444, sub)), (f, sub)


def test_upsampling_of_a_flat_plane_is_flat_and_linear_mirrors_the_halving():
    c = np.full((5, 7), 93, dtype=np.uint8)
    for sub, (w, h) in [(A.SUBSAMP_420, (13, 9)), (A.SUBSAMP_420, (14, 10)), (A.SUBSAMP_422, (13, 5))]:
        for mode in (RG.REPLICATE, RG.LINEAR):
            assert (RG.upsample(c, w, h, sub, mode) == 93).all()
    ramp = np.array([[0, 40, 80, 120]], dtype=np.uint8)
    assert RG.upsample(ramp, 8, 1, A.SUBSAMP_422, RG.LINEAR).tolist() == [[0, 10, 30, 50, 70, 90, 110, 120]]
    assert RG.upsample(ramp, 7, 1, A.SUBSAMP_422, RG.REPLICATE).tolist() == [[0, 0, 40, 40, 80, 80, 120]]
