"""The resampler on the GPU (include/dsv1_api.h dsv1_scale_clip, csrc/k_scale.hip) equals the numpy statement in tests/_scale.py byte
for byte: every format, both filters, the ratios 1, 4/3, 3/2, 2, 8/3, 4 and 8, odd plane sizes and sizes that are not multiples of the
64 x 16 tile, 4K to 1080p / 720p / 360p, host and device input."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import _scale as Z

pytestmark = pytest.mark.gpu

FORMATS = [A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411]
FILTERS = [Z.TENT, Z.CUBIC]


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return m


def clip_of(w, h, fmt, n, seed):
    """synthetic frames with detail and edges (the coder's generator) plus noise in the last frame: every tap matters"""
    c = A.gen_clip(w, h, fmt, seed, n, style=seed % 4).copy()
    c[-1] ^= np.random.default_rng(seed).integers(0, 256, c.shape[1], dtype=np.uint8)
    return c


def check(pkg, clip, sw, sh, fmt, dw, dh, f):
    got = pkg.scale_clip(clip, sw, sh, fmt, dw, dh, f)
    want = Z.scale_clip(clip, sw, sh, fmt, dw, dh, f)
    assert got.shape == want.shape
    bad = np.nonzero(got != want)
    assert bad[0].size == 0, "%dx%d -> %dx%d fmt %d filter %d: %d bytes differ, first at frame %d byte %d" % (
        sw, sh, fmt, dw, dh, f, bad[0].size, bad[0][0], bad[1][0])


# source 192 x 144 -> the ratios 1, 4/3, 3/2, 2, 8/3, 4, 8 (on both axes)
RATIOS = [(192, 144), (144, 108), (128, 96), (96, 72), (72, 54), (48, 36), (24, 18)]


@pytest.mark.parametrize("f", FILTERS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_ratios_formats_filters(pkg, fmt, f):
    clip = clip_of(192, 144, fmt, 3, 0x5C + fmt)
    for dw, dh in RATIOS:
        check(pkg, clip, 192, 144, fmt, dw, dh, f)


@pytest.mark.parametrize("f", FILTERS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("sw,sh,dw,dh", [(199, 147, 67, 55), (131, 77, 131, 77), (130, 91, 17, 13), (333, 65, 250, 9), (65, 17, 65, 3),
                                         (97, 40, 13, 39), (8, 8, 1, 1), (1, 1, 1, 1)])
def test_odd_and_untiled_sizes(pkg, fmt, f, sw, sh, dw, dh):
    if pkg.lib().dsv1_scale_taps(A.chroma_dims(sw, sh, fmt)[0], A.chroma_dims(dw, dh, fmt)[0], f) < 0 or \
       pkg.lib().dsv1_scale_taps(A.chroma_dims(sw, sh, fmt)[1], A.chroma_dims(dw, dh, fmt)[1], f) < 0:
        with pytest.raises(RuntimeError, match="rc=-2"):          # (a chroma axis beyond 8:1: refused, not scaled)
            pkg.scale_clip(clip_of(sw, sh, fmt, 1, 3), sw, sh, fmt, dw, dh, f)
        return
    check(pkg, clip_of(sw, sh, fmt, 2, sw * 7 + sh), sw, sh, fmt, dw, dh, f)


def test_4k(pkg):
    w, h, fmt = 3840, 2160, A.SUBSAMP_420
    clip = clip_of(w, h, fmt, 2, 0x4C)
    for dw, dh in [(1920, 1080), (1280, 720), (640, 360)]:
        check(pkg, clip, w, h, fmt, dw, dh, Z.CUBIC)
    check(pkg, clip[:1], w, h, fmt, 1280, 720, Z.TENT)


@pytest.mark.parametrize("f", FILTERS)
def test_device_input(pkg, f):
    """device pointers in and out (n frames), the source at an odd offset and the result at an odd offset as well"""
    sw, sh, dw, dh, fmt, n = 250, 130, 166, 86, A.SUBSAMP_420, 3
    clip = clip_of(sw, sh, fmt, n, 0xDE)
    L = pkg.lib()
    b = pkg.Batch(pkg.make_encoder_cfg(64, 64, fmt), 1, 1)            # (a context to allocate device memory through)
    try:
        sfb, dfb = A.frame_bytes(sw, sh, fmt), A.frame_bytes(dw, dh, fmt)
        src = b.upload(np.concatenate([np.zeros(1, np.uint8), clip.reshape(-1)]))
        dst = C.c_void_p(None)
        assert L.dsvg_dev_alloc(b.ctx, C.byref(dst), n * dfb + 1) == 0
        b._dev.append(dst)
        pkg.scale_clip(C.c_void_p(src.value + 1), sw, sh, fmt, dw, dh, f, n=n, out=C.c_void_p(dst.value + 1))
        got = np.zeros(n * dfb + 1, dtype=np.uint8)
        assert L.dsvg_dev_download(b.ctx, got.ctypes.data, dst, got.size) == 0
        assert np.array_equal(got[1:].reshape(n, dfb), Z.scale_clip(clip, sw, sh, fmt, dw, dh, f))
        assert sfb * n > 0
    finally:
        b.close()
