"""Source pixel formats on the host (no GPU): dsv1_pix_frame_bytes against the numpy statement in tests/_pixfmt.py over the whole
matrix, every invalid combination, the argument errors of every new entry point (which come before any device is looked at), and
tests/_pixfmt.py against itself: round trips, the tie and clamp values of the depth reduction, the ignored bits."""
import ctypes as C
import importlib
import itertools

import numpy as np
import pytest

import _cabi as A
import _pixfmt as PF

DSVG_ERR_ARG = -2
NODEV = 1 << 20          # a device number no machine has: a call that passes the checks fails there, not with DSVG_ERR_ARG
GEOMS = [(352, 288), (250, 130), (100, 36), (33, 17)]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("digital-subband-video-1_amd")


def cpf(pkg, f):
    return pkg.PixFormat(f["layout"], f["depth"], f["msb"], f["pitch"], f["frame_bytes"])


def paddings(f, w, h, fmt):
    """the format tight, with padded pitches, with a padded frame stride (dicts); f must be valid"""
    lay, planes, _ = PF.plane_layout(f, w, h, fmt)
    pitch = tuple(lay[k][2] + (5, 16, 7)[k] if k < len(lay) else 0 for k in range(3))
    return [f, dict(f, pitch=pitch), dict(f, frame_bytes=planes + 37), dict(f, pitch=pitch, frame_bytes=PF.plane_layout(dict(f, pitch=pitch), w, h, fmt)[1] + 64)]


def matrix():
    for layout, depth, msb, fmt in itertools.product(PF.LAYOUTS, PF.DEPTHS, (0, 1), PF.SUBSAMPS):
        if depth == 8 and msb:
            continue
        yield PF.pf(layout, depth, msb), fmt


def test_frame_bytes_equals_numpy_over_the_matrix(pkg):
    L = pkg.lib()
    nvalid = ninvalid = 0
    for f, fmt in matrix():
        for w, h in GEOMS:
            if not PF.valid(f["layout"], f["depth"], fmt):
                assert PF.frame_bytes(f, w, h, fmt) == 0
                assert L.dsv1_pix_frame_bytes(C.byref(cpf(pkg, f)), w, h, fmt) == 0, (f, fmt)
                ninvalid += 1
                continue
            for g in paddings(f, w, h, fmt):
                want = PF.frame_bytes(g, w, h, fmt)
                assert want > 0
                assert L.dsv1_pix_frame_bytes(C.byref(cpf(pkg, g)), w, h, fmt) == want, (g, w, h, fmt)
                assert pkg.pix_frame_bytes(cpf(pkg, g), w, h, fmt) == want
                nvalid += 1
    assert nvalid > 500 and ninvalid > 100


def test_tight_sizes_are_the_known_ones():
    w, h = 1920, 1080
    assert PF.frame_bytes(PF.pf(PF.SEMI_UV), w, h, A.SUBSAMP_420) == w * h * 3 // 2                # NV12
    assert PF.frame_bytes(PF.pf(PF.SEMI_UV, 10, 1), w, h, A.SUBSAMP_420) == w * h * 3              # P010
    assert PF.frame_bytes(PF.pf(PF.YUYV), w, h, A.SUBSAMP_422) == w * h * 2                        # YUY2
    assert PF.frame_bytes(PF.pf(PF.PLANAR, 10, 0), w, h, A.SUBSAMP_422) == w * h * 4               # yuv422p10le
    assert PF.frame_bytes(PF.pf(), 33, 17, A.SUBSAMP_420) == A.frame_bytes(33, 17, A.SUBSAMP_420)


def invalid_formats(w, h, fmt420=A.SUBSAMP_420):
    """(format, subsampling): every kind of invalid combination include/dsv1_api.h lists"""
    out = [(PF.pf(5), fmt420), (PF.pf(-1), fmt420), (PF.pf(PF.PLANAR, 9), fmt420), (PF.pf(PF.PLANAR, 0), fmt420), (PF.pf(PF.PLANAR, 14), fmt420),
           (PF.pf(PF.PLANAR, 10, 2), fmt420), (PF.pf(PF.PLANAR, 10, -1), fmt420),
           (PF.pf(PF.SEMI_UV), A.SUBSAMP_444), (PF.pf(PF.SEMI_VU, 10, 1), A.SUBSAMP_411),
           (PF.pf(PF.YUYV), fmt420), (PF.pf(PF.UYVY), A.SUBSAMP_444), (PF.pf(PF.YUYV, 10, 1), A.SUBSAMP_422), (PF.pf(PF.UYVY, 16, 0), A.SUBSAMP_422),
           (PF.pf(PF.PLANAR), 3), (PF.pf(PF.PLANAR), 0x10),
           (PF.pf(PF.PLANAR, pitch=(w - 1, 0, 0)), fmt420), (PF.pf(PF.PLANAR, pitch=(0, 0, 1)), fmt420), (PF.pf(PF.PLANAR, pitch=(-w, 0, 0)), fmt420),
           (PF.pf(PF.PLANAR, 10, 0, pitch=(2 * w - 1, 0, 0)), fmt420),
           (PF.pf(PF.SEMI_UV, pitch=(0, 2 * ((w + 1) // 2) - 1, 0)), fmt420), (PF.pf(PF.SEMI_UV, 10, 1, pitch=(0, 2 * w - 1, 0)), fmt420),
           (PF.pf(PF.YUYV, pitch=(4 * ((w + 1) // 2) - 1, 0, 0)), A.SUBSAMP_422),
           (PF.pf(PF.SEMI_UV, frame_bytes=w * h), fmt420), (PF.pf(PF.PLANAR, frame_bytes=A.frame_bytes(w, h, fmt420) - 1), fmt420)]
    return out


def test_invalid_combinations_give_zero(pkg):
    L = pkg.lib()
    for w, h in GEOMS:
        for f, fmt in invalid_formats(w, h):
            assert PF.frame_bytes(f, w, h, fmt) == 0, (f, fmt)
            assert L.dsv1_pix_frame_bytes(C.byref(cpf(pkg, f)), w, h, fmt) == 0, (f, w, h, fmt)
    nv12 = cpf(pkg, PF.pf(PF.SEMI_UV))
    for w, h in [(0, 16), (16, 0), (-4, 16)]:
        assert L.dsv1_pix_frame_bytes(C.byref(nv12), w, h, A.SUBSAMP_420) == 0
    assert L.dsv1_pix_frame_bytes(None, 64, 64, A.SUBSAMP_420) == 0
    with pytest.raises(ValueError):
        pkg.pix_frame_bytes(cpf(pkg, PF.pf(PF.YUYV)), 64, 64, A.SUBSAMP_420)


def test_convert_clip_arguments(pkg):
    L = pkg.lib()
    w, h, fmt = 64, 48, A.SUBSAMP_420
    nv12 = cpf(pkg, PF.pf(PF.SEMI_UV))
    src = np.zeros(2 * PF.frame_bytes(PF.pf(PF.SEMI_UV), w, h, fmt), dtype=np.uint8)
    dst = np.zeros(2 * A.frame_bytes(w, h, fmt), dtype=np.uint8)
    s, d = src.ctypes.data, dst.ctypes.data
    for f, sub in invalid_formats(w, h):
        assert L.dsv1_convert_clip(NODEV, s, C.byref(cpf(pkg, f)), w, h, sub, 1, d, 0) == DSVG_ERR_ARG, (f, sub)
    for args in [(NODEV, None, C.byref(nv12), w, h, fmt, 1, d, 0), (NODEV, s, None, w, h, fmt, 1, d, 0), (NODEV, s, C.byref(nv12), w, h, fmt, 1, None, 0),
                 (NODEV, s, C.byref(nv12), w, h, fmt, 0, d, 0), (NODEV, s, C.byref(nv12), 0, h, fmt, 1, d, 0), (-1, s, C.byref(nv12), w, h, fmt, 1, d, 0)]:
        assert L.dsv1_convert_clip(*args) == DSVG_ERR_ARG
    for f, sub, ww, hh in [(PF.pf(PF.SEMI_UV), fmt, w, h), (PF.pf(PF.PLANAR, 10, 0), A.SUBSAMP_411, 33, 17), (PF.pf(PF.UYVY), A.SUBSAMP_422, 33, 17)]:
        assert L.dsv1_convert_clip(NODEV, s, C.byref(cpf(pkg, f)), ww, hh, sub, 1, d, 0) not in (0, DSVG_ERR_ARG)    # odd sizes are the converter's too
    with pytest.raises(ValueError):
        pkg.convert_clip(src[:-1], nv12, w, h, fmt)


def test_batch_set_source_format_arguments(pkg):
    L = pkg.lib()
    assert L.dsv1_batch_set_source_format(None, C.byref(cpf(pkg, PF.pf(PF.SEMI_UV)))) == DSVG_ERR_ARG
    assert L.dsv1_batch_set_source_format(None, None) == DSVG_ERR_ARG


# ---- dsv1_resladder_open_src ---------------------------------------------------------------------------------------------------
SW, SH, FMT = 640, 360, A.SUBSAMP_420


def rl_open_src(pkg, f, geoms, src=(SW, SH, FMT), nsources=1, F=4, filt=1, device=NODEV, null=()):
    L = pkg.lib()
    arrs = [(pkg.Encoder * max(len(r), 1))(*r) for _, _, r in geoms]
    rr = (pkg.ResRung * max(len(geoms), 1))(*[pkg.ResRung(w, h, len(r), a) for (w, h, r), a in zip(geoms, arrs)])
    meta = pkg.Meta()
    meta.width, meta.height, meta.subsamp = src
    hnd = C.c_void_p(None)
    rc = L.dsv1_resladder_open_src(None if "out" in null else C.byref(hnd), None if "src" in null else C.byref(meta),
                                   None if f is None else C.byref(cpf(pkg, f)), None if "rungs" in null else rr, len(geoms), device, nsources, F, filt)
    assert not hnd.value
    return rc


def geo(pkg, w, h, qps=(85,), fmt=FMT):
    return (w, h, [pkg.make_encoder_cfg(w, h, fmt, qp=q, gop=12, rc_mode_cli=1) for q in qps])


def test_resladder_open_src_arguments(pkg):
    ok = [geo(pkg, SW, SH), geo(pkg, 320, 180, (60, 90))]
    for f in (None, PF.pf(), PF.pf(PF.SEMI_UV), PF.pf(PF.SEMI_UV, 10, 1, pitch=(2 * SW + 64, 2 * SW + 64, 0)), PF.pf(PF.PLANAR, 10, 0)):
        rc = rl_open_src(pkg, f, ok)
        assert rc not in (0, DSVG_ERR_ARG), (f, rc)                 # past the checks, to the device
    for f, sub in invalid_formats(SW, SH):
        if sub == FMT:
            assert rl_open_src(pkg, f, ok) == DSVG_ERR_ARG, f
    assert rl_open_src(pkg, PF.pf(PF.YUYV), ok) == DSVG_ERR_ARG      # packed needs 4:2:2
    for null in ("out", "src", "rungs"):
        assert rl_open_src(pkg, PF.pf(PF.SEMI_UV), ok, null=(null,)) == DSVG_ERR_ARG
    # and with a format the ladder's own refusals stay: upscaled rung, another subsampling, bad filter, bad counts
    nv12 = PF.pf(PF.SEMI_UV)
    assert rl_open_src(pkg, nv12, [geo(pkg, SW + 16, SH)]) == DSVG_ERR_ARG
    assert rl_open_src(pkg, nv12, [geo(pkg, 320, 180, fmt=A.SUBSAMP_422)]) == DSVG_ERR_ARG
    assert rl_open_src(pkg, nv12, ok, filt=2) == DSVG_ERR_ARG
    assert rl_open_src(pkg, nv12, ok, nsources=0) == DSVG_ERR_ARG


def test_resladder_open_keeps_its_refusals(pkg):
    """dsv1_resladder_open is open_src with the default format: what tests/test_scale_host.py says it refuses, it refuses"""
    L = pkg.lib()

    def rl_open(geoms, filt=1):
        arrs = [(pkg.Encoder * len(r))(*r) for _, _, r in geoms]
        rr = (pkg.ResRung * len(geoms))(*[pkg.ResRung(w, h, len(r), a) for (w, h, r), a in zip(geoms, arrs)])
        meta = pkg.Meta()
        meta.width, meta.height, meta.subsamp = SW, SH, FMT
        hnd = C.c_void_p(None)
        return L.dsv1_resladder_open(C.byref(hnd), C.byref(meta), rr, len(geoms), NODEV, 1, 4, filt)

    assert rl_open([geo(pkg, 320, 180, fmt=A.SUBSAMP_444)]) == DSVG_ERR_ARG
    assert rl_open([geo(pkg, SW * 2, SH * 2)]) == DSVG_ERR_ARG
    assert rl_open([geo(pkg, 320, 180)], filt=7) == DSVG_ERR_ARG
    assert rl_open([geo(pkg, 320, 180)]) not in (0, DSVG_ERR_ARG)


def test_python_input_sizes_follow_the_format(pkg):
    r = pkg.ResLadder.__new__(pkg.ResLadder)
    p010 = cpf(pkg, PF.pf(PF.SEMI_UV, 10, 1))
    r.nsources, r.F, r.frame_bytes = 2, 3, pkg.pix_frame_bytes(p010, SW, SH, FMT)
    assert r.frame_bytes == 2 * A.frame_bytes(SW, SH, FMT)
    assert r._input(np.zeros((2, 3, r.frame_bytes), dtype=np.uint8)).size == 6 * r.frame_bytes
    with pytest.raises(ValueError):
        r._input(np.zeros((2, 3, A.frame_bytes(SW, SH, FMT)), dtype=np.uint8))


# ---- tests/_pixfmt.py against itself -------------------------------------------------------------------------------------------
def valid_cases():
    for f, fmt in matrix():
        if PF.valid(f["layout"], f["depth"], fmt):
            yield f, fmt


@pytest.mark.parametrize("w,h", [(64, 48), (33, 17), (250, 130)])
def test_round_trip(w, h):
    rng = np.random.default_rng(w * h)
    for f, fmt in valid_cases():
        x = rng.integers(0, 256, (2, A.frame_bytes(w, h, fmt)), dtype=np.uint8)
        for g in paddings(f, w, h, fmt):
            vals = x if g["depth"] == 8 else PF.widen(x, g["depth"])
            buf = PF.pack(vals, g, w, h, fmt, rng)
            assert buf.size == 2 * PF.frame_bytes(g, w, h, fmt)
            assert np.array_equal(PF.convert(buf, g, w, h, fmt, 2), x), (g, fmt)


@pytest.mark.parametrize("d", [10, 12, 16])
@pytest.mark.parametrize("msb", [0, 1])
def test_tie_and_clamp_values(d, msb):
    def one(v):
        x = (v << (16 - d)) if msb else v
        return int(PF.reduce_depth(np.array([x], dtype=np.uint16), d, msb)[0])

    assert one((1 << d) - 1) == 255                    # would round to 256: clamped
    assert one(1 << (d - 9)) == 1                      # the tie rounds up
    assert one((1 << (d - 9)) - 1) == 0
    assert one(0) == 0 and one(255 << (d - 8)) == 255 and one(128 << (d - 8)) == 128
    assert one((254 << (d - 8)) + (1 << (d - 9))) == 255
    # every value against the definition written out with Python integers
    v = np.arange(1 << d, dtype=np.int64)
    x = ((v << (16 - d)) if msb else v).astype(np.uint16)
    want = np.minimum(255, (v + (1 << (d - 9))) >> (d - 8))
    assert np.array_equal(PF.reduce_depth(x, d, msb), want)


@pytest.mark.parametrize("d", [10, 12])
def test_unused_bits_change_nothing(d):
    w, h, fmt = 40, 24, A.SUBSAMP_420
    rng = np.random.default_rng(d)
    v = rng.integers(0, 1 << d, (1, A.frame_bytes(w, h, fmt)), dtype=np.uint32)
    for layout in (PF.PLANAR, PF.SEMI_UV):
        for msb in (0, 1):
            f = PF.pf(layout, d, msb)
            clean = PF.pack(v, f, w, h, fmt, np.random.default_rng(3), garbage=False)
            dirty = PF.pack(v, f, w, h, fmt, np.random.default_rng(3), garbage=True)
            assert not np.array_equal(clean, dirty)
            assert np.array_equal(PF.convert(clean, f, w, h, fmt, 1), PF.convert(dirty, f, w, h, fmt, 1))
            assert np.array_equal(PF.convert(clean, f, w, h, fmt, 1)[0], PF.reduce_depth((v[0] << (16 - d)) if msb else v[0], d, msb))
