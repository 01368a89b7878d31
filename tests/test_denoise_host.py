"""The temporal noise filter's definition (tests/_denoise.py, the numpy statement of include/dsv1_api.h, Temporal noise reduction) has
the properties the header promises, the clips the GPU tests use reach every branch of it, it buys what it is for, and
dsv1_denoise_state_bytes and the validator work without a device."""
import ctypes as C

import numpy as np
import pytest

import _cabi as A
import _denoise as D

DSVG_ERR_ARG = -2
FMTS = [A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411]


class Denoise(C.Structure):
    _fields_ = [("luma", C.c_int), ("chroma", C.c_int)]


def prod():
    L = A.load_prod()
    L.dsv1_denoise_state_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    L.dsv1_denoise_state_bytes.restype = C.c_size_t
    L.dsv1_denoise_valid.argtypes = [C.POINTER(Denoise)]
    L.dsv1_denoise_clip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Denoise), C.c_int]
    return L


@pytest.mark.parametrize("fmt", FMTS)
def test_state_bytes_and_validator_without_a_device(fmt):
    L = prod()
    for w, h in ((352, 288), (35, 19), (1, 1), (1920, 1080)):
        assert L.dsv1_denoise_state_bytes(w, h, fmt) == D.state_bytes(w, h, fmt) == 3 * A.frame_bytes(w, h, fmt)
    assert L.dsv1_denoise_state_bytes(0, 4, fmt) == 0 and L.dsv1_denoise_state_bytes(4, -1, fmt) == 0 and L.dsv1_denoise_state_bytes(4, 4, 0x7) == 0
    buf = np.zeros(4096, dtype=np.uint8)
    for luma, chroma in ((24, 24), (1, 0), (0, 1), (512, 512), (0, 512), (-1, 4), (4, -1), (513, 4), (4, 513), (0, 0), (-1, -1), (1 << 20, 0)):
        dn = Denoise(luma, chroma)
        assert bool(L.dsv1_denoise_valid(C.byref(dn))) == D.valid(luma, chroma), (luma, chroma)
        if not D.valid(luma, chroma):                    # the standalone call refuses it before it looks for a device
            assert L.dsv1_denoise_clip(0, buf.ctypes.data, 4, 4, fmt, 1, None, None, buf.ctypes.data, C.byref(dn), 0) == DSVG_ERR_ARG
    assert L.dsv1_denoise_valid(None) == 0
    ok = Denoise(24, 24)
    assert L.dsv1_denoise_clip(0, buf.ctypes.data, 4, 4, fmt, 1, None, None, buf.ctypes.data, None, 0) == DSVG_ERR_ARG
    assert L.dsv1_denoise_clip(0, buf.ctypes.data, 0, 4, fmt, 1, None, None, buf.ctypes.data, C.byref(ok), 0) == DSVG_ERR_ARG
    assert L.dsv1_denoise_clip(0, buf.ctypes.data, 4, 4, fmt, 0, None, None, buf.ctypes.data, C.byref(ok), 0) == DSVG_ERR_ARG
    assert L.dsv1_denoise_clip(0, buf.ctypes.data, 4, 4, 0x7, 1, None, None, buf.ctypes.data, C.byref(ok), 0) == DSVG_ERR_ARG


def test_a_noiseless_static_clip_comes_out_unchanged():
    w, h, fmt = 37, 21, A.SUBSAMP_420
    frame = np.random.default_rng(3).integers(0, 256, A.frame_bytes(w, h, fmt), dtype=np.uint8)
    clip = np.stack([frame] * 5)
    for luma, chroma in D.GPU_STRENGTHS:
        out, state = D.denoise_clip(clip, w, h, fmt, luma, chroma)
        assert np.array_equal(out, clip), (luma, chroma)
        again, _ = D.denoise_clip(clip[:2], w, h, fmt, luma, chroma, state=state)
        assert np.array_equal(again, clip[:2])


def test_a_sample_in_motion_is_the_input_and_restarts_its_state():
    w, h, fmt, T = 24, 16, A.SUBSAMP_444, 20
    rng = np.random.default_rng(4)
    a = rng.integers(0, 256, (3, A.frame_bytes(w, h, fmt)), dtype=np.uint8)
    out, state = D.denoise_clip(a, w, h, fmt, T, T)
    S = state[a.shape[1]:].view("<u2")
    st = {}
    D.denoise_clip(a, w, h, fmt, T, T, stats=st)
    assert st["moving"] > 0.99 * st["filtered"]          # (uniform noise: almost every sample moves)
    moved = np.ones(a.shape[1], dtype=bool)
    for o, (pw, ph) in zip((0, w * h, 2 * w * h), D.plane_dims(w, h, fmt)):
        d = np.pad(np.abs(a[2, o:o + pw * ph].astype(int) - a[1, o:o + pw * ph].astype(int)).reshape(ph, pw), 1, mode="edge")
        m0 = sum(d[1 + dy:1 + dy + ph, 1 + dx:1 + dx + pw] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
        moved[o:o + pw * ph] = (m0 >= 2 * T).reshape(-1)
    assert moved.mean() > 0.9
    assert np.array_equal(out[2][moved], a[2][moved]) and np.array_equal(S[moved], 16 * a[2][moved].astype(np.uint16))


def test_S_stays_within_its_range_on_a_uniformly_random_clip():
    w, h, fmt = 40, 23, A.SUBSAMP_422
    clip = np.random.default_rng(7).integers(0, 256, (8, A.frame_bytes(w, h, fmt)), dtype=np.uint8)
    clip[3:5] = np.where(clip[3:5] & 1, 255, 0)          # (the extremes, in every neighbourhood)
    for T in (1, 24, 200, 512):
        st = {}
        _, state = D.denoise_clip(clip, w, h, fmt, T, T, stats=st)
        assert 0 <= st["smin"] and st["smax"] <= 4080, (T, st)
        assert state[clip.shape[1]:].view("<u2").max() <= 4080


@pytest.mark.parametrize("strength", [(24, 24), (40, 0), (0, 16)])
def test_a_cut_stream_equals_the_uncut_one(strength):
    w, h, fmt, n = 33, 18, A.SUBSAMP_420, 6
    clip = D.gen_noisy(w, h, fmt, n, 5)
    whole, end = D.denoise_clip(clip, w, h, fmt, *strength)
    assert not np.array_equal(whole, clip)
    for cut in range(1, n):
        head, state = D.denoise_clip(clip[:cut], w, h, fmt, *strength)
        tail, end2 = D.denoise_clip(clip[cut:], w, h, fmt, *strength, state=state)
        assert np.array_equal(np.concatenate([head, tail]), whole), cut
        assert np.array_equal(end2, end), cut
    fb = clip.shape[1]
    if strength[1] == 0:                                 # a plane that is copied keeps no state: zeros
        assert not end[w * h:fb].any() and not end[fb + 2 * w * h:].any()


def test_the_gain_is_one_line_in_binary32():
    """csrc/k_denoise.hip computes k as trunc(fma(m, 12 / T, 4 - 12 + (T / 2 + 0.5) / T)) clamped to 4 .. 16: exact for every T and every
    m a picture can make (9 * 255), with and without the fusion"""
    m = np.arange(0, 9 * 255 + 1, dtype=np.int64)
    for T in range(1, D.T_MAX + 1):
        want = D.gain(m, T)
        a, b = np.float32(12.0 / T), np.float32(4.0 - 12.0 + (T // 2 + 0.5) / T)
        split = (m.astype(np.float32) * a).astype(np.float32) + b
        fused = (m.astype(np.float64) * np.float64(a) + np.float64(b)).astype(np.float32)
        for v in (split, fused):
            assert np.array_equal(np.clip(np.trunc(v).astype(np.int64), 4, 16), want), T


def coverage(cases, strengths):
    """counted on exactly what tests/test_gpu_denoise.py gives the device: D.gpu_case's pictures, from no state and from the state the
    picture before them left"""
    st = {}
    for w, h, fmt in cases:
        frames, before = D.gpu_case(w, h, fmt)
        for luma, chroma in strengths:
            _, state = D.denoise_clip(before[None], w, h, fmt, luma, chroma)
            D.denoise_clip(frames, w, h, fmt, luma, chroma, stats=st)
            D.denoise_clip(frames, w, h, fmt, luma, chroma, state=state, stats=st)
    return st


@pytest.mark.parametrize("cases,strengths", [(D.GPU_GEOMS, D.GPU_STRENGTHS), (D.GPU_GEOMS[:1], D.GPU_STRENGTHS), (D.GPU_GEOMS[1:2], D.GPU_STRENGTHS)],
                         ids=["all", "352x288", "250x130"])
def test_the_gpu_tests_clips_reach_every_branch(cases, strengths):
    """instrumented statement: m <= T, T < m < 2 T, m >= 2 T, and 3 |c - pout| > m0, each on at least 1 % of the filtered samples"""
    st = coverage(cases, strengths)
    assert st["still"] + st["between"] + st["moving"] == st["filtered"]
    for k in ("still", "between", "moving", "recursive"):
        assert st[k] >= 0.01 * st["filtered"], (k, st)


def test_it_buys_what_it_is_for():
    """a static scene loses its noise, a moving one is left alone (no ghosting), a clean one is untouched"""
    w, h, fmt, n = 96, 128, A.SUBSAMP_420, 12
    clean, noisy = D.gen_scene(w, h, fmt, n, 5, 2.0, 0.0)
    out, _ = D.denoise_clip(noisy, w, h, fmt, 24, 24)
    gain = D.psnr(out[6:], clean[6:]) - D.psnr(noisy[6:], clean[6:])
    print("static: %.2f dB in, %+.2f dB" % (D.psnr(noisy[6:], clean[6:]), gain))
    assert gain >= 4.0
    clean, noisy = D.gen_scene(w, h, fmt, n, 5, 2.0, 2.5)
    out, _ = D.denoise_clip(noisy, w, h, fmt, 24, 24)
    loss = D.psnr(noisy[6:], clean[6:]) - D.psnr(out[6:], clean[6:])
    print("moving: %.2f dB in, %+.2f dB" % (D.psnr(noisy[6:], clean[6:]), -loss))
    assert loss <= 0.25
    clean, _ = D.gen_scene(w, h, fmt, n, 5, 0.0, 0.0)
    assert np.array_equal(D.denoise_clip(clean, w, h, fmt, 24, 24)[0], clean)
