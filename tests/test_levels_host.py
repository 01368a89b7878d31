"""Levels and histograms without a device (include/dsv1_api.h, Levels): the table builders equal the exact-rational statement
tests/_levels.py over their whole domain, the end points the header names are pinned as literals, the range and point rules equal
numpy on random histograms, and the standalone calls refuse invalid input before they look for a device."""
import ctypes as C
import itertools

import numpy as np

import _cabi as A
import _levels as LV

DSVG_ERR_ARG = -2
NO_DEVICE = 4096                                          # a device index no machine has


class Levels(C.Structure):
    _fields_ = [("lut", (C.c_uint8 * 256) * 3)]


def prod():
    L = A.load_prod()
    P = C.POINTER(Levels)
    L.dsv1_levels_identity.argtypes = [P]
    L.dsv1_levels_range.argtypes = [P, C.c_int, C.c_int]
    L.dsv1_levels_adjust.argtypes = [P] + [C.c_int] * 5
    L.dsv1_levels_compose.argtypes = [P, P, P]
    L.dsv1_levels_is_identity.argtypes = [P]
    L.dsv1_range_from_histogram.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.dsv1_points_from_histogram.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.dsv1_levels_clip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, P, C.c_int]
    L.dsv1_histogram_clip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.dsv1_detect_range_clip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    return L


def tab(lv):
    return np.frombuffer(bytes(lv), dtype=np.uint8).reshape(3, 256).copy()


def filled(v=0xA5):
    lv = Levels()
    C.memset(C.byref(lv), v, 768)
    return lv


def of(t):
    lv = Levels()
    t = np.ascontiguousarray(t, dtype=np.uint8)
    C.memmove(C.byref(lv), t.ctypes.data, 768)
    return lv


def test_the_struct_is_768_bytes_in_the_headers_order():
    hdr = open(A.ROOT + "/include/dsv1_api.h").read()
    assert "typedef struct { uint8_t lut[3][256]; } dsv1_levels;" in hdr
    assert C.sizeof(Levels) == 768


def test_identity():
    L = prod()
    lv = filled()
    assert L.dsv1_levels_identity(C.byref(lv)) == 0
    assert np.array_equal(tab(lv), LV.identity()) and L.dsv1_levels_is_identity(C.byref(lv)) == 1
    for p, v in ((0, 0), (1, 128), (2, 255)):
        t = LV.identity()
        t[p, v] ^= 1
        assert L.dsv1_levels_is_identity(C.byref(of(t))) == 0
    assert L.dsv1_levels_identity(None) == DSVG_ERR_ARG and L.dsv1_levels_is_identity(None) == 0


def test_range_equals_the_statement():
    L = prod()
    for s, d in itertools.product((0, 1), repeat=2):
        lv = filled()
        assert L.dsv1_levels_range(C.byref(lv), s, d) == 0
        A.assert_same("range(%d, %d)" % (s, d), tab(lv), LV.range_(s, d))
        assert L.dsv1_levels_is_identity(C.byref(lv)) == (s == d)


def test_range_end_points():
    L = prod()
    lv = Levels()
    assert L.dsv1_levels_range(C.byref(lv), 1, 0) == 0
    t = tab(lv)
    assert (t[0, 0], t[0, 255]) == (16, 235)
    assert (t[1, 0], t[1, 255]) == (16, 240) and (t[2, 0], t[2, 255]) == (16, 240)
    assert t[1, 128] == 128 and t[2, 128] == 128
    assert L.dsv1_levels_range(C.byref(lv), 0, 1) == 0
    t = tab(lv)
    assert (t[0, 16], t[0, 235]) == (0, 255) and (t[0, 0], t[0, 255]) == (0, 255)         # the clamp binds on the luma outside 16 .. 235
    assert (t[1, 16], t[1, 240]) == (1, 255) and (t[2, 16], t[2, 240]) == (1, 255)         # chroma 16 gives 1, chroma 240 gives 255
    assert t[1, 128] == 128


def test_range_is_monotone_and_round_trips_within_one():
    L = prod()
    down, up, both = Levels(), Levels(), Levels()
    assert L.dsv1_levels_range(C.byref(down), 1, 0) == 0 and L.dsv1_levels_range(C.byref(up), 0, 1) == 0
    t = tab(down).astype(int)
    assert (np.diff(t, axis=1) >= 0).all()
    assert L.dsv1_levels_compose(C.byref(down), C.byref(up), C.byref(both)) == 0
    assert (np.abs(tab(both).astype(int) - np.arange(256)) <= 1).all()
    A.assert_same("compose", tab(both), LV.compose(LV.range_(1, 0), LV.range_(0, 1)))


ADJ_IN = [(0, 1), (0, 255), (254, 255), (16, 235), (10, 11), (100, 200), (0, 128)]
ADJ_OUT = [(0, 0), (0, 255), (255, 255), (16, 235), (7, 8), (200, 201)]
ADJ_SAT = [0, 1, 128, 255, 256, 257, 300, 512, 1023, 1024]


def test_adjust_equals_the_statement():
    L = prod()
    for (ib, iw), (ob, ow), sat in itertools.product(ADJ_IN, ADJ_OUT, ADJ_SAT):
        lv = filled()
        assert L.dsv1_levels_adjust(C.byref(lv), ib, iw, ob, ow, sat) == 0, (ib, iw, ob, ow, sat)
        assert np.array_equal(tab(lv), LV.adjust(ib, iw, ob, ow, sat)), (ib, iw, ob, ow, sat)
    lv = Levels()
    assert L.dsv1_levels_adjust(C.byref(lv), 0, 255, 0, 255, 256) == 0 and L.dsv1_levels_is_identity(C.byref(lv)) == 1
    assert L.dsv1_levels_adjust(C.byref(lv), 0, 255, 0, 255, 0) == 0
    assert (tab(lv)[1:] == 128).all() and np.array_equal(tab(lv)[0], np.arange(256))


def test_invalid_arguments_leave_the_tables_untouched():
    L = prod()
    before = filled(0x5A)
    lv = filled(0x5A)
    bad_adjust = [(-1, 255, 0, 255, 256), (0, 256, 0, 255, 256), (10, 10, 0, 255, 256), (11, 10, 0, 255, 256), (255, 255, 0, 255, 256),
                  (0, 255, -1, 255, 256), (0, 255, 0, 256, 256), (0, 255, 9, 8, 256), (0, 255, 0, 255, -1), (0, 255, 0, 255, 1025),
                  (0, 0, 0, 0, 0), (1 << 30, 1 << 30, 0, 0, 0)]
    for a in bad_adjust:
        assert not LV.adjust_valid(*a)
        assert L.dsv1_levels_adjust(C.byref(lv), *a) == DSVG_ERR_ARG, a
        assert bytes(lv) == bytes(before), a
    for s, d in ((-1, 0), (0, -1), (2, 0), (0, 2), (2, 2), (-1, -1), (1, 256)):
        assert LV.range_(s, d) is None
        assert L.dsv1_levels_range(C.byref(lv), s, d) == DSVG_ERR_ARG, (s, d)
        assert bytes(lv) == bytes(before)
    assert L.dsv1_levels_adjust(None, 0, 255, 0, 255, 256) == DSVG_ERR_ARG and L.dsv1_levels_range(None, 0, 1) == DSVG_ERR_ARG
    assert L.dsv1_levels_compose(None, C.byref(lv), C.byref(lv)) == DSVG_ERR_ARG
    assert L.dsv1_levels_compose(C.byref(lv), None, C.byref(lv)) == DSVG_ERR_ARG
    assert L.dsv1_levels_compose(C.byref(lv), C.byref(lv), None) == DSVG_ERR_ARG
    assert bytes(lv) == bytes(before)


def test_compose_with_aliased_arguments():
    L = prod()
    ta, tb = LV.random_tables(1), LV.random_tables(2)
    want = LV.compose(ta, tb)
    assert not np.array_equal(want, LV.compose(tb, ta))
    a, b, out = of(ta), of(tb), Levels()
    assert L.dsv1_levels_compose(C.byref(a), C.byref(b), C.byref(out)) == 0 and np.array_equal(tab(out), want)
    assert np.array_equal(tab(a), ta) and np.array_equal(tab(b), tb)
    a = of(ta)
    assert L.dsv1_levels_compose(C.byref(a), C.byref(b), C.byref(a)) == 0 and np.array_equal(tab(a), want)          # out is a
    a, b = of(ta), of(tb)
    assert L.dsv1_levels_compose(C.byref(a), C.byref(b), C.byref(b)) == 0 and np.array_equal(tab(b), want)          # out is b
    a = of(ta)
    assert L.dsv1_levels_compose(C.byref(a), C.byref(a), C.byref(a)) == 0 and np.array_equal(tab(a), LV.compose(ta, ta))


def rule_range(L, hist, ppm):
    g = np.ascontiguousarray(hist, dtype=np.uint32)
    full = C.c_int(-7)
    rc = L.dsv1_range_from_histogram(g.ctypes.data, g.size // 768, ppm, C.byref(full))
    return rc, full.value


def rule_points(L, hist, lo, hi):
    g = np.ascontiguousarray(hist, dtype=np.uint32)
    b, w = C.c_int(-7), C.c_int(-7)
    rc = L.dsv1_points_from_histogram(g.ctypes.data, g.size // 768, lo, hi, C.byref(b), C.byref(w))
    return rc, b.value, w.value


def histograms():
    rng = np.random.default_rng(0x415)
    out = []
    for n in (1, 3):
        out.append(rng.integers(0, 5000, size=(n, 3, 256), dtype=np.uint32))
        g = rng.integers(0, 2000, size=(n, 3, 256), dtype=np.uint32)                     # a limited-range clip with a few strays
        g[:, 0, :16] //= 500; g[:, 0, 236:] //= 500; g[:, 1:, :16] //= 500; g[:, 1:, 241:] //= 500
        out.append(g)
        g = np.zeros((n, 3, 256), dtype=np.uint32)                                       # sharp peaks
        g[:, 0, 40], g[:, 0, 41], g[:, 0, 200], g[:, 1, 128], g[:, 2, 128] = 1000, 3, 999000, 250000, 250000
        out.append(g)
        out.append(np.full((n, 3, 256), 0xFFFFFFFF, dtype=np.uint32))                    # every count at its largest
    for v in (0, 15, 16, 128, 235, 236, 255):                                            # all samples in one bin
        g = np.zeros((1, 3, 256), dtype=np.uint32)
        g[0, 0, v], g[0, 1, v], g[0, 2, v] = 2073600, 518400, 518400
        out.append(g)
    for v in (240, 241):
        g = np.zeros((2, 3, 256), dtype=np.uint32)
        g[:, 0, 100], g[:, 1, v], g[:, 2, v] = 64, 16, 16
        out.append(g)
    return out


PPMS = (0, 1, 999, 1000, 500000, 999999, 1000000)


def test_range_from_histogram_equals_numpy():
    L = prod()
    seen = set()
    for g in histograms():
        for ppm in PPMS:
            want = LV.range_from_histogram(g, ppm)
            assert rule_range(L, g, ppm) == (0, int(want)), ppm
            seen.add(want)
    assert seen == {False, True}
    g = histograms()[0]
    for ppm in (-1, 1000001):
        assert rule_range(L, g, ppm) == (DSVG_ERR_ARG, -7)
    full = C.c_int(-7)
    assert L.dsv1_range_from_histogram(g.ctypes.data, 0, 1000, C.byref(full)) == DSVG_ERR_ARG
    assert L.dsv1_range_from_histogram(g.ctypes.data, -1, 1000, C.byref(full)) == DSVG_ERR_ARG
    assert L.dsv1_range_from_histogram(None, 1, 1000, C.byref(full)) == DSVG_ERR_ARG
    assert L.dsv1_range_from_histogram(g.ctypes.data, 1, 1000, None) == DSVG_ERR_ARG
    # exactly on the bound is not "more than": 1 sample in a million outside at ppm 1
    g = np.zeros((1, 3, 256), dtype=np.uint32)
    g[0, 0, 100], g[0, 0, 5] = 999999, 1
    assert rule_range(L, g, 1) == (0, 0) and rule_range(L, g, 0) == (0, 1)


def test_points_from_histogram_equals_numpy():
    L = prod()
    found = {True: 0, False: 0}
    for g in histograms():
        for lo, hi in itertools.product(PPMS, repeat=2):
            want = LV.points_from_histogram(g, lo, hi)
            rc, b, w = rule_points(L, g, lo, hi)
            assert (rc, b, w) == ((1,) + want if want else (0, 0, 0)), (lo, hi)
            found[want is not None] += 1
    assert found[True] and found[False]
    # literals: a ramp with one sample per value
    g = np.zeros((1, 3, 256), dtype=np.uint32)
    g[0, 0, :] = 1
    assert rule_points(L, g, 0, 0) == (1, 0, 255)
    assert rule_points(L, g, 62500, 62500) == (1, 16, 239)                               # 16 of 256 samples on each side
    assert rule_points(L, g, 1000000, 1000000) == (0, 0, 0)                              # black 255, white 0: black >= white
    one = np.zeros((1, 3, 256), dtype=np.uint32)
    one[0, 0, 77] = 12345
    assert rule_points(L, one, 0, 0) == (0, 0, 0)                                        # all samples in one bin: black = white = 77
    g = histograms()[0]
    for lo, hi in ((-1, 0), (0, -1), (1000001, 0), (0, 1000001)):
        assert rule_points(L, g, lo, hi) == (DSVG_ERR_ARG, 0, 0)
    b, w = C.c_int(-7), C.c_int(-7)
    assert L.dsv1_points_from_histogram(g.ctypes.data, 0, 0, 0, C.byref(b), C.byref(w)) == DSVG_ERR_ARG
    assert L.dsv1_points_from_histogram(None, 1, 0, 0, C.byref(b), C.byref(w)) == DSVG_ERR_ARG
    assert L.dsv1_points_from_histogram(g.ctypes.data, 1, 0, 0, None, C.byref(w)) == DSVG_ERR_ARG
    assert L.dsv1_points_from_histogram(g.ctypes.data, 1, 0, 0, C.byref(b), None) == DSVG_ERR_ARG


def test_the_statement_of_the_pass_and_the_histogram():
    """tests/_levels.py against a loop over the samples, at a geometry whose planes have odd sizes"""
    fmt, w, h = A.SUBSAMP_420, 5, 3
    clip = LV.noise(2, w, h, fmt, 9)
    t = LV.random_tables(3)
    out = LV.levels_clip(clip, w, h, fmt, t)
    hist = LV.histogram(clip, w, h, fmt)
    cw, ch = A.chroma_dims(w, h, fmt)
    assert (cw, ch) == (3, 2) and clip.shape == (2, 27)
    for f in range(2):
        count = np.zeros((3, 256), dtype=np.uint32)
        for i in range(27):
            p = 0 if i < 15 else 1 if i < 21 else 2
            assert out[f, i] == t[p, clip[f, i]]
            count[p, clip[f, i]] += 1
        assert np.array_equal(hist[f], count)
    assert hist.dtype == np.uint32 and [int(hist[0, p].sum()) for p in range(3)] == [15, 6, 6]


def test_the_standalone_calls_refuse_before_they_look_for_a_device():
    L = prod()
    fmt, w, h = A.SUBSAMP_420, 8, 6
    src = LV.noise(1, w, h, fmt, 1)
    dst = np.full_like(src, 0x5A)
    hist = np.full((1, 3, 256), 0x5A5A5A5A, dtype=np.uint32)
    lv = of(LV.random_tables(4))
    full = C.c_int(-7)
    lev = lambda **k: L.dsv1_levels_clip(k.get("dev", NO_DEVICE), k.get("src", src.ctypes.data), k.get("w", w), k.get("h", h), k.get("fmt", fmt),
                                         k.get("n", 1), k.get("dst", dst.ctypes.data), k.get("lv", C.byref(lv)), 0)
    his = lambda **k: L.dsv1_histogram_clip(k.get("dev", NO_DEVICE), k.get("src", src.ctypes.data), k.get("w", w), k.get("h", h), k.get("fmt", fmt),
                                            k.get("n", 1), k.get("hist", hist.ctypes.data), 0)
    det = lambda **k: L.dsv1_detect_range_clip(k.get("dev", NO_DEVICE), k.get("src", src.ctypes.data), k.get("w", w), k.get("h", h), k.get("fmt", fmt),
                                               k.get("n", 1), k.get("ppm", 1000), k.get("full", C.byref(full)), 0)
    common = [dict(src=None), dict(n=0), dict(n=-1), dict(w=0), dict(h=0), dict(w=-3), dict(dev=-1), dict(fmt=0x7), dict(fmt=0x1), dict(fmt=-1)]
    for bad in common + [dict(dst=None), dict(lv=None)]:
        assert lev(**bad) == DSVG_ERR_ARG, bad
    for bad in common + [dict(hist=None)]:
        assert his(**bad) == DSVG_ERR_ARG, bad
    for bad in common + [dict(full=None), dict(ppm=-1), dict(ppm=1000001)]:
        assert det(**bad) == DSVG_ERR_ARG, bad
    for call in (lev, his, det):
        rc = call()
        assert rc < 0 and rc != DSVG_ERR_ARG              # valid arguments: only now is the device missed
    assert (dst == 0x5A).all() and (hist == 0x5A5A5A5A).all() and full.value == -7
