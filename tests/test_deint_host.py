"""The deinterlacer's definition (tests/_deint.py, the numpy statement of include/dsv1_api.h, Deinterlacing) has the properties the
header promises, the clip generator the GPU tests use reaches every branch of it, and dsv1_deint_out_frames validates its arguments
without a device."""
import ctypes as C

import numpy as np
import pytest

import _cabi as A
import _deint as D

DSVG_ERR_ARG = -2
MODES = [D.FRAME, D.FIELD]


def noise_clip(w, h, fmt, n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, A.frame_bytes(w, h, fmt)), dtype=np.uint8)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tff", [0, 1])
def test_static_clip_is_woven_from_its_second_frame_on(mode, tff):
    w, h, fmt = 37, 21, A.SUBSAMP_420
    frame = noise_clip(w, h, fmt, 1, 3)[0]
    clip = np.stack([frame] * 4)
    out = D.deint_clip(clip, w, h, fmt, mode, tff)
    per = 2 if mode == D.FIELD else 1
    assert out.shape[0] == D.out_frames(mode, 4) == 4 * per
    assert not np.array_equal(out[0], frame)             # (noise: the first frame's made lines are interpolated)
    for k in range(per, out.shape[0]):
        assert np.array_equal(out[k], frame), k
    assert np.array_equal(D.deint_clip(clip[:2], w, h, fmt, mode, tff, prev=frame), clip[:2].repeat(per, axis=0))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tff", [0, 1])
def test_kept_lines_are_the_inputs(mode, tff):
    w, h, fmt = 40, 23, A.SUBSAMP_422
    clip = D.gen_interlaced(w, h, fmt, 3, 11, tff)
    out = D.deint_clip(clip, w, h, fmt, mode, tff)
    p = 0 if tff else 1
    per = 2 if mode == D.FIELD else 1
    for k in range(out.shape[0]):
        q = p if k % per == 0 else 1 - p
        for a, b in zip(D.planes_of(clip[k // per], w, h, fmt), D.planes_of(out[k], w, h, fmt)):
            assert np.array_equal(a[q::2], b[q::2])


@pytest.mark.parametrize("mode", MODES)
def test_a_cut_stream_equals_the_uncut_one(mode):
    w, h, fmt, n = 33, 18, A.SUBSAMP_420, 5
    clip = D.gen_interlaced(w, h, fmt, n, 5)
    whole = D.deint_clip(clip, w, h, fmt, mode, 1)
    per = 2 if mode == D.FIELD else 1
    for cut in range(1, n):
        head = D.deint_clip(clip[:cut], w, h, fmt, mode, 1)
        tail = D.deint_clip(clip[cut:], w, h, fmt, mode, 1, prev=clip[cut - 1])
        assert np.array_equal(np.concatenate([head, tail]), whole), cut
        assert head.shape[0] == cut * per


@pytest.mark.parametrize("w,h,fmt", [(16, 2, A.SUBSAMP_420), (9, 1, A.SUBSAMP_444), (1, 1, A.SUBSAMP_420)])
def test_planes_of_one_row_are_copied(w, h, fmt):
    clip = noise_clip(w, h, fmt, 3, 9)
    for mode in MODES:
        out = D.deint_clip(clip, w, h, fmt, mode, 0, prev=clip[2])
        per = 2 if mode == D.FIELD else 1
        for k in range(out.shape[0]):
            for pl, (a, b) in enumerate(zip(D.planes_of(clip[k // per], w, h, fmt), D.planes_of(out[k], w, h, fmt))):
                if a.shape[0] == 1:
                    assert np.array_equal(a, b), (k, pl)


def coverage(cases, modes=MODES):
    """counted on exactly what tests/test_gpu_deint.py gives the device: D.gpu_case's frames, without and with its `prev`"""
    st = {}
    for w, h, fmt in cases:
        for mode in modes:
            for tff in (0, 1):
                frames, before = D.gpu_case(w, h, fmt, tff)
                for prev in (None, before):
                    D.deint_clip(frames, w, h, fmt, mode, tff, prev=prev, stats=st)
    return st


@pytest.mark.parametrize("cases", [D.GPU_GEOMS[:1], D.GPU_GEOMS[1:2], D.GPU_GEOMS], ids=["352x288", "250x130", "all"])
def test_the_gpu_tests_clips_reach_every_branch(cases):
    """instrumented statement: every direction wins on at least 0.5 % of the made samples, every clamp outcome occurs on at least 5 %
    -- for the two large geometries on their own and over the whole list"""
    st = coverage(cases)
    for j in D.DIRS:
        assert st[("dir", j)] >= 0.005 * st["made"], (j, st)
    for k in ("below", "inside", "above"):
        assert st[k] >= 0.05 * st["clamped"], (k, st)
    assert st["below"] + st["inside"] + st["above"] == st["clamped"]


def test_out_frames_validates_without_a_device():
    L = A.load_prod()

    class Deint(C.Structure):
        _fields_ = [("mode", C.c_int), ("tff", C.c_int)]

    L.dsv1_deint_out_frames.argtypes = [C.POINTER(Deint), C.c_int]
    assert L.dsv1_deint_out_frames(C.byref(Deint(0, 0)), 7) == 7
    assert L.dsv1_deint_out_frames(C.byref(Deint(0, 1)), 0) == 0
    assert L.dsv1_deint_out_frames(C.byref(Deint(1, 1)), 7) == 14
    assert L.dsv1_deint_out_frames(C.byref(Deint(1, 0)), (1 << 30) - 1) == (1 << 31) - 2
    for bad in (Deint(2, 0), Deint(-1, 1), Deint(0, 2), Deint(1, -1)):
        assert L.dsv1_deint_out_frames(C.byref(bad), 4) == DSVG_ERR_ARG
    assert L.dsv1_deint_out_frames(None, 4) == DSVG_ERR_ARG
    assert L.dsv1_deint_out_frames(C.byref(Deint(0, 0)), -1) == DSVG_ERR_ARG
    assert L.dsv1_deint_out_frames(C.byref(Deint(1, 0)), 1 << 30) == DSVG_ERR_ARG       # 2n does not fit
    # the standalone call refuses the same before it looks for a device
    L.dsv1_deinterlace_clip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Deint), C.c_int]
    buf = np.zeros(64, dtype=np.uint8)
    for bad in (Deint(2, 0), Deint(0, 2)):
        assert L.dsv1_deinterlace_clip(0, buf.ctypes.data, 4, 4, A.SUBSAMP_420, 1, None, buf.ctypes.data, C.byref(bad), 0) == DSVG_ERR_ARG
    assert L.dsv1_deinterlace_clip(0, buf.ctypes.data, 4, 4, 0x7, 1, None, buf.ctypes.data, C.byref(Deint(0, 1)), 0) == DSVG_ERR_ARG
    assert L.dsv1_deinterlace_clip(0, buf.ctypes.data, 0, 4, A.SUBSAMP_420, 1, None, buf.ctypes.data, C.byref(Deint(0, 1)), 0) == DSVG_ERR_ARG
