"""The resampler in both directions on the host (no GPU): the C weight tables (dsv1_resample_weights) equal the numpy statement in
tests/_resample.py for many (S, D) pairs up and down, equal dsv1_scale_weights bit for bit where S >= D, are the identity where
S == D and keep the kernel's int32 bounds; the limits are refused; and the argument errors of the source-resolution calls of
resolution ladders come back before any device is looked at."""
import ctypes as C
import importlib
import random

import numpy as np
import pytest

import _cabi as A
import _resample as RS
import _scale as Z

DSVG_ERR_ARG = -2
NODEV = 1 << 20          # a device number no machine has
FILTERS = [RS.TENT, RS.CUBIC]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("digital-subband-video-1_amd")


def pairs():
    """(S, D) both ways: every integer ratio 1..8 either way, many in between, odd sizes"""
    rnd = random.Random(0x0B5CA1E)
    out = set()
    for n in list(range(1, 24)) + [45, 77, 127, 135, 270, 360, 480, 511, 540, 720]:
        for r in range(1, 9):
            if n * r <= 4096:
                out |= {(n * r, n), (n, n * r)}
        for _ in range(4):
            m = rnd.randint(max(1, (n + 7) // 8), min(8 * n, 4096))
            out |= {(m, n), (n, m)}
    while len(out) < 900:
        D = rnd.randint(1, 4096)
        S = rnd.randint(max(1, (D + 7) // 8), min(8 * D, 4096))
        out.add((S, D))
    out |= {(1280, 1920), (720, 1080), (960, 1920), (540, 1080), (640, 960), (360, 540), (1919, 1920), (1, 8), (3, 17)}
    return sorted(out)


PAIRS = pairs()


def test_tables_equal_numpy_both_ways(pkg):
    bad = []
    for S, D in PAIRS:
        for f in FILTERS:
            assert pkg.resample_taps(S, D, f) == RS.taps(S, D, f)
            cs, cq = pkg.resample_weights(S, D, f)
            ns, nq = RS.weights(S, D, f)
            if not (np.array_equal(cs, ns) and np.array_equal(cq, nq)):
                bad.append((S, D, f))
    assert sum(S < D for S, D in PAIRS) > 300
    assert not bad, "C and numpy tables differ at %s" % bad[:5]


def test_downscale_tables_are_the_scalers_bit_for_bit(pkg):
    n = 0
    for S, D in PAIRS:
        if S < D:
            continue
        for f in FILTERS:
            assert pkg.resample_taps(S, D, f) == pkg.scale_taps(S, D, f)
            a, b = pkg.resample_weights(S, D, f), pkg.scale_weights(S, D, f)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (S, D, f)
            n += 1
    assert n > 500


@pytest.mark.parametrize("f", FILTERS)
@pytest.mark.parametrize("n", [1, 2, 7, 100, 1080])
def test_same_size_is_the_identity(pkg, f, n):
    start, q = pkg.resample_weights(n, n, f)
    for i in range(n):
        nz = np.nonzero(q[i])[0]
        assert len(nz) == 1 and q[i, nz[0]] == RS.ONE and start[i] + nz[0] == i
    P = np.random.default_rng(n).integers(0, 256, (min(n, 37), n), dtype=np.uint8)
    assert np.array_equal(RS.resample_plane(P, n, P.shape[0], f), P)


@pytest.mark.parametrize("f", FILTERS)
def test_rows_sum_to_one_and_starts_rise(f):
    for S, D in PAIRS[::2]:
        start, q = RS.weights(S, D, f)
        assert (q.astype(np.int64).sum(axis=1) == RS.ONE).all(), (S, D)
        assert (np.diff(start.astype(np.int64)) >= 0).all(), (S, D)


def test_int32_bound_of_every_table():
    """sum |q| < 2 * 16384 in every row of every table both ways (the bound k_scale / k_xres_quality use for |H|, |Hs|, |V|)"""
    worst = 0
    for S, D in PAIRS:
        for f in FILTERS:
            _, q = RS.weights(S, D, f)
            worst = max(worst, int(np.abs(q.astype(np.int64)).sum(axis=1).max()))
    assert worst < 2 * RS.ONE
    hs_max = ((255 * worst + 128) >> 8) + 1
    assert hs_max < 2 ** 15 and hs_max * worst < 2 ** 31


@pytest.mark.parametrize("f", FILTERS)
@pytest.mark.parametrize("v", [0, 1, 128, 255])
def test_constant_plane_stays_constant_upscaled(f, v):
    for (w, h), (dw, dh) in [((21, 17), (64, 48)), ((5, 4), (37, 29)), ((13, 99), (100, 100)), ((2, 2), (16, 16))]:
        assert (RS.resample_plane(np.full((h, w), v, dtype=np.uint8), dw, dh, f) == v).all()


def test_limits_are_refused(pkg):
    L = pkg.lib()
    for S, D, f in [(9, 1, 0), (1, 9, 0), (17, 2, 1), (2, 17, 1), (0, 5, 0), (5, 0, 0), (5, 5, 2), (5, 5, -1)]:
        assert L.dsv1_resample_taps(S, D, f) == DSVG_ERR_ARG, (S, D, f)
    assert L.dsv1_resample_taps(1, 8, 0) == 4 and L.dsv1_resample_taps(1, 8, 1) == 6 and L.dsv1_resample_taps(8, 1, 1) == 34
    assert L.dsv1_scale_taps(1, 2, 0) == DSVG_ERR_ARG              # the downscaler's contract is unchanged
    q = np.zeros(64, dtype=np.int16)
    s = np.zeros(16, dtype=np.int32)
    assert L.dsv1_resample_weights(8, 16, 1, s.ctypes.data, q.ctypes.data, 5) == DSVG_ERR_ARG     # T is not that axis's
    with pytest.raises(ValueError):
        pkg.resample_taps(10, 100, 1)


def test_resample_clip_arguments(pkg):
    L = pkg.lib()
    fmt = A.SUBSAMP_420
    a = np.zeros(A.frame_bytes(32, 32, fmt), dtype=np.uint8)
    o = np.zeros(A.frame_bytes(64, 64, fmt), dtype=np.uint8)
    for sw, sh, fm, n, dw, dh, f in [(32, 32, fmt, 1, 257, 32, 1), (32, 32, fmt, 1, 3, 32, 1), (32, 32, fmt, 0, 64, 64, 1),
                                     (32, 32, 3, 1, 64, 64, 1), (32, 32, fmt, 1, 64, 64, 2)]:
        assert L.dsv1_resample_clip(NODEV, a.ctypes.data, sw, sh, fm, n, o.ctypes.data, dw, dh, f, 0) == DSVG_ERR_ARG
    # an upscale passes the checks (and fails at the device); dsv1_scale_clip still refuses it
    assert L.dsv1_resample_clip(NODEV, a.ctypes.data, 32, 32, fmt, 1, o.ctypes.data, 64, 64, 1, 0) not in (0, DSVG_ERR_ARG)
    assert L.dsv1_scale_clip(NODEV, a.ctypes.data, 32, 32, fmt, 1, o.ctypes.data, 64, 64, 1, 0) == DSVG_ERR_ARG
    with pytest.raises(ValueError):
        pkg.resample_clip(np.zeros(A.frame_bytes(32, 32, fmt) + 1, dtype=np.uint8), 32, 32, fmt, 64, 64)


def test_src_quality_argument_errors_before_a_device(pkg):
    """no handle: every source-resolution call is an argument error, and nothing touches a device"""
    L = pkg.lib()
    assert L.dsv1_resladder_src_quality_enable(None, 1, 1, 1) == DSVG_ERR_ARG
    buf = (C.c_uint64 * 12)()
    fx = (C.c_int64 * 12)()
    assert L.dsv1_resladder_get_src_sse(None, buf, 12) == DSVG_ERR_ARG
    assert L.dsv1_resladder_get_src_ssim(None, fx, 12) == DSVG_ERR_ARG
    # and a resolution ladder that cannot open (no such device) leaves no handle to call them with
    meta = pkg.Meta()
    meta.width, meta.height, meta.subsamp = 320, 180, A.SUBSAMP_420
    encs = (pkg.Encoder * 1)(pkg.make_encoder_cfg(160, 90, A.SUBSAMP_420, qp=80, gop=12, rc_mode_cli=1))
    rr = (pkg.ResRung * 1)(pkg.ResRung(160, 90, 1, encs))
    h = C.c_void_p(None)
    assert L.dsv1_resladder_open(C.byref(h), C.byref(meta), rr, 1, NODEV, 1, 4, 1) not in (0, DSVG_ERR_ARG)
    assert not h.value


def test_numpy_upscale_matches_a_plain_statement():
    """a 2x tent upscale of a ramp stays within the ramp and keeps its ends: the statement's grids are centre-aligned"""
    P = np.tile(np.arange(0, 160, 10, dtype=np.uint8), (4, 1))
    U = RS.resample_plane(P, 32, 8, RS.TENT)
    assert U[:, 0].max() == 0 and U[:, -1].min() == 150
    assert (np.diff(U.astype(int), axis=1) >= 0).all()
    assert np.array_equal(RS.resample_plane(P, 16, 4, RS.CUBIC), Z.scale_plane(P, 16, 4, Z.CUBIC))
