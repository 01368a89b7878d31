"""Inverse telecine and field order detection without a device (include/dsv1_api.h, Inverse telecine): the struct, the sizes, the two
decision rules (the ones the kernels compile, csrc/dsvg_ivtc_rules.h) and the vote equal the numpy statement tests/_ivtc.py; the ties
fall as the header says; the model itself recovers the film frames of clean telecined clips; every entry point refuses invalid input
before it looks for a device."""
import ctypes as C

import numpy as np
import pytest

import _cabi as A
import _ivtc as I

DSVG_ERR_ARG = -2
NO_DEVICE = 4096                                          # a device index no machine has
U32MAX = 0xFFFFFFFF


class Ivtc(C.Structure):
    _fields_ = [("tff", C.c_int), ("nt", C.c_int), ("reserved", C.c_int * 2)]

    def __init__(self, tff=1, nt=0, reserved=(0, 0)):
        super().__init__(tff, nt, (C.c_int * 2)(*reserved))


def prod():
    L = A.load_prod()
    L.dsv1_ivtc_out_frames.argtypes = [C.POINTER(Ivtc), C.c_int]
    L.dsv1_ivtc_state_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    L.dsv1_ivtc_state_bytes.restype = C.c_size_t
    L.dsv1_field_metrics_clip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.dsv1_field_order_from_metrics.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.dsv1_detect_field_order_clip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.dsv1_ivtc_match.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.dsv1_ivtc_pick.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.dsv1_ivtc_clip.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Ivtc),
                                 C.c_void_p, C.c_void_p, C.c_int]
    L.dsv1_batch_set_source_ivtc.argtypes = [C.c_void_p, C.POINTER(Ivtc)]
    L.dsv1_batch_ivtc_reset.argtypes = [C.c_void_p, C.c_int]
    L.dsv1_resladder_set_ivtc.argtypes = [C.c_void_p, C.POINTER(Ivtc)]
    L.dsv1_resladder_ivtc_reset.argtypes = [C.c_void_p, C.c_int]
    return L


def c_match(L, met, first_has_prev, tff):
    met = np.ascontiguousarray(met, dtype=np.uint32)
    out = np.full(met.shape[0], 7, dtype=np.uint8)
    assert L.dsv1_ivtc_match(met.ctypes.data, met.shape[0], first_has_prev, tff, out.ctypes.data) == 0
    return out


def c_pick(L, D):
    D = np.ascontiguousarray(D, dtype=np.uint32)
    out = np.full(D.size // 5, 7, dtype=np.uint8)
    assert L.dsv1_ivtc_pick(D.ctypes.data, D.size, out.ctypes.data) == 0
    return out


def c_order(L, met, first_has_prev=0):
    met = np.ascontiguousarray(met, dtype=np.uint32)
    return L.dsv1_field_order_from_metrics(met.ctypes.data, met.shape[0], first_has_prev)


def test_the_struct_is_the_headers():
    assert C.sizeof(Ivtc) == 16 and Ivtc.nt.offset == 4 and Ivtc.reserved.offset == 8


def test_struct_validation_and_out_frames():
    L = prod()
    for tff in (0, 1):
        for nt in (0, 8, 254):
            for n in (0, 5, 10, 65535 * 5):
                assert L.dsv1_ivtc_out_frames(C.byref(Ivtc(tff, nt)), n) == 4 * n // 5
    good = Ivtc(1, 0)
    for n in (-5, -1, 1, 4, 6, 9, 11):
        assert L.dsv1_ivtc_out_frames(C.byref(good), n) == DSVG_ERR_ARG
    for bad in (Ivtc(2, 0), Ivtc(-1, 0), Ivtc(1, -1), Ivtc(1, 255), Ivtc(1, 0, (1, 0)), Ivtc(0, 0, (0, 1))):
        assert L.dsv1_ivtc_out_frames(C.byref(bad), 10) == DSVG_ERR_ARG
    assert L.dsv1_ivtc_out_frames(None, 10) == DSVG_ERR_ARG


def test_state_bytes():
    L = prod()
    for w, h in ((352, 288), (35, 19), (1, 1), (64, 3), (1920, 1080)):
        for fmt in (A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411):
            assert L.dsv1_ivtc_state_bytes(w, h, fmt) == A.frame_bytes(w, h, fmt) + w * h == I.state_bytes(w, h, fmt)
    assert L.dsv1_ivtc_state_bytes(0, 4, A.SUBSAMP_420) == 0 and L.dsv1_ivtc_state_bytes(4, -1, A.SUBSAMP_420) == 0
    assert L.dsv1_ivtc_state_bytes(4, 4, 0x7) == 0


def seeded_metrics(seed, n):
    """metric tables with small values, so that equal pairs are frequent, and a few at the top of the range"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 4, (n, 4)).astype(np.uint32)
    big = rng.random((n, 4)) < 0.2
    m[big] = rng.integers(U32MAX - 2, U32MAX + 1, int(big.sum())).astype(np.uint32)
    return m


@pytest.mark.parametrize("seed", range(6))
def test_match_equals_the_model(seed):
    L = prod()
    met = seeded_metrics(seed, 40)
    for tff in (0, 1):
        for fhp in (0, 1):
            got = c_match(L, met, fhp, tff)
            assert (got == I.match_of(met, bool(fhp), tff)).all()
            assert set(got) <= {I.C, I.P}
    # both outcomes and an equal pair occur in the table, or the comparison shows little
    p0 = I.match_of(met, True, 1)
    assert (p0 == I.P).any() and (p0 == I.C).any() and (met[:, 2] == met[:, 0]).any()


def test_match_ties_and_first_picture():
    L = prod()
    met = np.array([[5, 9, 5, 9], [5, 9, 4, 8], [5, 9, 6, 10], [0, 0, 0, 0], [U32MAX, 0, U32MAX - 1, 0]], dtype=np.uint32)
    # tff reads (mc0, mp0), bff (mc1, mp1); equal mp and mc: C; strictly less: P
    assert list(c_match(L, met, 1, 1)) == [I.C, I.P, I.C, I.C, I.P]
    assert list(c_match(L, met, 1, 0)) == [I.C, I.P, I.C, I.C, I.C]
    # a first picture without prv is C whatever its numbers say
    assert list(c_match(L, met[1:2], 0, 1)) == [I.C] and list(c_match(L, met[1:2], 1, 1)) == [I.P]
    out = np.zeros(5, dtype=np.uint8)
    assert L.dsv1_ivtc_match(None, 5, 0, 1, out.ctypes.data) == DSVG_ERR_ARG
    assert L.dsv1_ivtc_match(met.ctypes.data, 5, 0, 1, None) == DSVG_ERR_ARG
    assert L.dsv1_ivtc_match(met.ctypes.data, 5, 0, 2, out.ctypes.data) == DSVG_ERR_ARG
    assert L.dsv1_ivtc_match(met.ctypes.data, -1, 0, 1, out.ctypes.data) == DSVG_ERR_ARG


@pytest.mark.parametrize("seed", range(6))
def test_pick_equals_the_model(seed):
    L = prod()
    rng = np.random.default_rng(100 + seed)
    D = rng.integers(0, 3, 50).astype(np.uint32)
    D[rng.random(50) < 0.15] = U32MAX
    assert (c_pick(L, D) == I.pick_of(D)).all()


def test_pick_ties():
    L = prod()
    # equal D drops the earliest
    assert list(c_pick(L, [3, 3, 3, 3, 3])) == [0]
    assert list(c_pick(L, [4, 2, 9, 2, 2])) == [1]
    assert list(c_pick(L, [4, 5, 9, 7, 2])) == [4]
    # a first picture (UINT32_MAX) is never dropped unless all five tie
    assert list(c_pick(L, [U32MAX, U32MAX - 1, U32MAX, U32MAX, U32MAX])) == [1]
    assert list(c_pick(L, [U32MAX, 0, 0, 0, 0])) == [1]
    assert list(c_pick(L, [U32MAX] * 5)) == [0]
    # cycles are independent
    assert list(c_pick(L, [U32MAX, 7, 7, 8, 9, 0, 1, 2, 3, 4, 9, 9, 9, 9, 1])) == [1, 0, 4]
    out = np.zeros(2, dtype=np.uint8)
    D = np.zeros(10, dtype=np.uint32)
    for n in (-5, 1, 4, 6, 9):
        assert L.dsv1_ivtc_pick(D.ctypes.data, n, out.ctypes.data) == DSVG_ERR_ARG
    assert L.dsv1_ivtc_pick(None, 10, out.ctypes.data) == DSVG_ERR_ARG and L.dsv1_ivtc_pick(D.ctypes.data, 10, None) == DSVG_ERR_ARG


def vote_table(tv, bv, quiet=2):
    """a metric table whose frames from the second on give tv tff votes, bv bff votes and `quiet` that vote for neither; the first frame
    would vote tff if it were counted"""
    rows = [[0, 0, 1, 2]] + [[0, 0, 1, 2]] * tv + [[0, 0, 2, 1]] * bv + [[0, 0, 3, 3]] * quiet
    return np.array(rows, dtype=np.uint32)


def test_the_vote_and_its_boundaries():
    L = prod()
    for tv, bv, want in ((1, 0, 1), (0, 1, 0), (0, 0, -1), (4, 2, -1), (5, 2, 1), (2, 4, -1), (2, 5, 0), (3, 3, -1), (12, 0, 1), (0, 12, 0),
                         (2, 1, -1), (3, 1, 1), (1, 2, -1), (1, 3, 0)):
        met = vote_table(tv, bv)
        assert I.votes_of(met) == (tv, bv)
        assert c_order(L, met) == want == I.field_order_of(met), (tv, bv)
    # the first frame counts only where it has a prv
    met = vote_table(2, 1)
    assert c_order(L, met, 0) == -1 and c_order(L, met, 1) == 1 == I.field_order_of(met, True)
    assert c_order(L, met[:1], 0) == -1 and c_order(L, met[:1], 1) == 1
    assert L.dsv1_field_order_from_metrics(None, 4, 0) == DSVG_ERR_ARG
    assert L.dsv1_field_order_from_metrics(met.ctypes.data, 0, 0) == DSVG_ERR_ARG


@pytest.mark.parametrize("seed", range(4))
def test_vote_equals_the_model_on_seeded_tables(seed):
    L = prod()
    met = seeded_metrics(200 + seed, 30)
    for fhp in (0, 1):
        assert c_order(L, met, fhp) == I.field_order_of(met, bool(fhp))


# ---- the numpy definition's own properties ----
@pytest.mark.parametrize("tff", (1, 0))
@pytest.mark.parametrize("phase", range(4))
@pytest.mark.parametrize("w,h,fmt", [(64, 48, A.SUBSAMP_420), (35, 19, A.SUBSAMP_444)])
def test_model_recovers_the_film_frames(w, h, fmt, phase, tff):
    """a clean telecined clip (20 frames, any of the four film frames of the pulldown cycle first, either order): the 16 kept pictures
    are the 16 film frames, byte for byte, however the stream is cut into calls"""
    film = I.film_frames(w, h, fmt, 16, 0x1F + phase)
    clip, seq = I.telecine(film, w, h, fmt, tff, phase)
    assert clip.shape[0] == 20
    out, match, drop, state, D = I.ivtc_clip(clip, w, h, fmt, tff)
    assert I.kept_film(seq, match, drop) == list(range(16))
    assert out.shape == film.shape and (out == film).all()
    assert (state[:A.frame_bytes(w, h, fmt)] == clip[-1]).all()
    # cut into calls of 5 and 15 with the state passed on: the same
    o1, m1, d1, s1, _ = I.ivtc_clip(clip[:5], w, h, fmt, tff)
    o2, m2, d2, s2, _ = I.ivtc_clip(clip[5:], w, h, fmt, tff, state=s1)
    assert (np.concatenate([o1, o2]) == out).all() and (np.concatenate([m1, m2]) == match).all() and (np.concatenate([d1, d2]) == drop).all()
    assert (s2 == state).all()
    # the vote: in every cycle three frames repeat a field of the frame before them, which weaves to nothing under the true order
    # only; the other two follow a whole film step and may fall either way, so the clip as a whole need not reach 2 : 1
    tv, bv = I.votes_of(I.field_metrics(clip, w, h))
    assert (tv if tff else bv) >= 12 and tv + bv <= 19


def test_model_with_the_wrong_order_does_not_recover_them():
    """the property above is the field order's doing: the same clip read with the other order keeps combed pictures"""
    w, h, fmt = 64, 48, A.SUBSAMP_420
    film = I.film_frames(w, h, fmt, 16, 0x1F)
    clip, seq = I.telecine(film, w, h, fmt, 1, 0)
    out = I.ivtc_clip(clip, w, h, fmt, 0)[0]
    assert not (out == film).all()


def test_model_static_clip():
    """static material: every match C (mp is never below mc = 0 ... both are equal), D = 0 but for the stream's first picture, so the
    first cycle of a stream drops picture 1 -- its first has UINT32_MAX -- and every later cycle picture 0"""
    w, h, fmt = 35, 19, A.SUBSAMP_420
    one = I.film_frames(w, h, fmt, 1, 3)
    clip = np.repeat(one, 15, axis=0)
    out, match, drop, state, D = I.ivtc_clip(clip, w, h, fmt, 1)
    assert (match == I.C).all() and list(drop) == [1, 0, 0] and D[0] == U32MAX and not D[1:].any()
    assert (out == np.repeat(one, 12, axis=0)).all()
    # static: what the frame before would supply is what the frame has, mp == mc
    met = I.field_metrics(clip, w, h)
    assert (met[1:, 2:] == met[1:, :2]).all()


def test_model_static_clip_does_not_vote():
    """a static clip without vertical detail: every metric is 0, no frame votes, the order is undetermined"""
    clip = I.static_columns(64, 48, A.SUBSAMP_420, 20, 9)
    met = I.field_metrics(clip, 64, 48)
    assert not met.any() and I.votes_of(met) == (0, 0) and I.field_order_of(met) == -1
    assert np.ptp(clip[0][:64 * 48].reshape(48, 64)[0]) > 50


@pytest.mark.parametrize("tff", (1, 0))
@pytest.mark.parametrize("speed", (1, 2))
def test_model_names_the_order_of_interlaced_pans(speed, tff):
    clip = I.interlaced_pan(64, 48, A.SUBSAMP_420, 20, 0x77, tff, speed)
    met = I.field_metrics(clip, 64, 48)
    assert I.field_order_of(met) == tff
    tv, bv = I.votes_of(met)
    assert (tv, bv) == ((19, 0) if tff else (0, 19))


# ---- refusals before any device is looked for ----
def test_clip_calls_refuse_bad_arguments_and_report_a_missing_device():
    L = prod()
    w, h, fmt = 16, 8, A.SUBSAMP_420
    fb = A.frame_bytes(w, h, fmt)
    clip = np.zeros((10, fb), dtype=np.uint8)
    dst = np.full((8, fb), 0x5A, dtype=np.uint8)
    met = np.full((10, 4), 0x5A5A5A5A, dtype=np.uint32)
    iv = Ivtc(1, 0)

    def ivtc(n=10, src=clip.ctypes.data, out=dst.ctypes.data, ww=w, hh=h, f=fmt, p=iv, dev=NO_DEVICE):
        return L.dsv1_ivtc_clip(dev, src, ww, hh, f, n, None, None, out, C.byref(p) if p is not None else None, None, None, 0)

    for kw in (dict(n=0), dict(n=4), dict(n=7), dict(n=-5), dict(src=None), dict(out=None), dict(ww=0), dict(hh=0), dict(f=0x7), dict(p=None),
               dict(p=Ivtc(2, 0)), dict(p=Ivtc(1, 255)), dict(p=Ivtc(1, 0, (0, 3))), dict(dev=-1), dict(ww=8192, hh=4096)):
        assert ivtc(**kw) == DSVG_ERR_ARG, kw
    assert ivtc() not in (0, DSVG_ERR_ARG)

    def fm(n=10, src=clip.ctypes.data, out=met.ctypes.data, ww=w, hh=h, f=fmt, nt=0, dev=NO_DEVICE):
        return L.dsv1_field_metrics_clip(dev, src, ww, hh, f, n, None, nt, out, 0)

    for kw in (dict(n=0), dict(src=None), dict(out=None), dict(ww=0), dict(hh=-1), dict(f=0x9), dict(nt=-1), dict(nt=255), dict(dev=-1),
               dict(ww=8192, hh=4096)):
        assert fm(**kw) == DSVG_ERR_ARG, kw
    assert fm() not in (0, DSVG_ERR_ARG)

    def fo(n=10, src=clip.ctypes.data, ww=w, hh=h, f=fmt, nt=0, dev=NO_DEVICE):
        return L.dsv1_detect_field_order_clip(dev, src, ww, hh, f, n, nt, 0)

    for kw in (dict(n=0), dict(src=None), dict(ww=0), dict(f=0x9), dict(nt=255), dict(dev=-1)):
        assert fo(**kw) == DSVG_ERR_ARG, kw
    assert fo() < -1                                       # an error, never one of the answers 1 / 0 / -1
    assert (dst == 0x5A).all() and (met == 0x5A5A5A5A).all()


def test_session_setters_refuse_null_sessions():
    L = prod()
    iv = Ivtc(1, 0)
    assert L.dsv1_batch_set_source_ivtc(None, C.byref(iv)) == DSVG_ERR_ARG and L.dsv1_batch_ivtc_reset(None, -1) == DSVG_ERR_ARG
    assert L.dsv1_resladder_set_ivtc(None, C.byref(iv)) == DSVG_ERR_ARG and L.dsv1_resladder_ivtc_reset(None, -1) == DSVG_ERR_ARG
