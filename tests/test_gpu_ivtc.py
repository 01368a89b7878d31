"""Inverse telecine and field order detection on the GPU (include/dsv1_api.h, Inverse telecine; csrc/k_ivtc.hip): the field metrics
equal the numpy statement tests/_ivtc.py integer for integer on the 16-byte path and on the byte path; dsv1_ivtc_clip equals it in
pictures, decisions and state, and gives back the film frames themselves; batches, quality ladders, chain mode and resolution
ladders with the pass set write the streams the oracle writes for the numpy result of the whole clip -- the state crosses the call
boundary."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import _denoise as DN
import _ivtc as I
import _pixfmt as PF
import _reframe as R
import _scale as Z

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2
CRF = dict(gop=4, rc_mode_cli=1, scd=1)
W, H, S, F = 64, 48, 2, 8                                 # sessions: frames_per_call 8 = 10 frames in per source and call
NCALLS = 3


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return m


class DevMem:
    """device memory through a small batch's context"""

    def __init__(self, pkg):
        self.b = pkg.Batch(pkg.make_encoder_cfg(64, 64, A.SUBSAMP_420), 1, 1)
        self.L = self.b.L

    def alloc(self, arr):
        return self.b.upload(arr)

    def read(self, p, nbytes):
        self.b.sync()
        out = np.zeros(nbytes, dtype=np.uint8)
        assert self.L.dsvg_dev_download(self.b.ctx, out.ctypes.data, p, nbytes) == 0
        return out

    def close(self):
        self.b.close()


@pytest.fixture(scope="module")
def mem(pkg):
    m = DevMem(pkg)
    yield m
    m.close()


# ---- field metrics -------------------------------------------------------------------------------------------------------------
# aligned 16-byte path; rows not 16-byte aligned; odd both ways; no interior line; one interior line; one sample; a row of 120 items
# over 8 runs: four blocks add into every sum
METRIC_GEOMS = [(352, 288, A.SUBSAMP_420), (250, 130, A.SUBSAMP_422), (35, 19, A.SUBSAMP_444), (16, 2, A.SUBSAMP_420), (64, 3, A.SUBSAMP_422),
                (1, 1, A.SUBSAMP_444), (1920, 64, A.SUBSAMP_420)]


@pytest.mark.parametrize("w,h,fmt", METRIC_GEOMS)
def test_field_metrics_equal_numpy(pkg, mem, w, h, fmt):
    n, fb = 3, A.frame_bytes(w, h, fmt)
    clip = I.add_noise(I.interlaced_pan(w, h, fmt, n + 1, 0xF1, 1, 2), 0xF2)
    frames, before = clip[1:], clip[0]
    for nt in (0, 8):
        for prev in (None, before):
            want = I.field_metrics(frames, w, h, prev, nt)
            got = pkg.field_metrics_clip(frames, w, h, fmt, prev=prev, nt=nt)
            assert got.dtype == np.uint32 and got.shape == (n, 4)
            assert np.array_equal(got, want), "host nt %d prev %s\n%s\n%s" % (nt, prev is not None, got, want)
            if h < 3:
                assert not want.any()
            elif prev is None:
                assert not want[0, 2:].any() and want[1:, 2:].any()
            # device memory, 16-byte aligned (the 16-byte path where the geometry allows it) and not (the byte path for every geometry)
            for off in (4096, 4096 + 3):
                big_s = np.full(off + n * fb + 4096, 0xC3, dtype=np.uint8)
                big_s[off:off + n * fb] = frames.reshape(-1)
                big_p = np.full(off + fb + 4096, 0x5A, dtype=np.uint8)
                big_p[off:off + fb] = before
                ps, pp = mem.alloc(big_s), mem.alloc(big_p)
                got = pkg.field_metrics_clip(C.c_void_p(ps.value + off), w, h, fmt, prev=C.c_void_p(pp.value + off) if prev is not None else None,
                                             nt=nt, n=n)
                assert np.array_equal(got, want), "device nt %d prev %s offset %d" % (nt, prev is not None, off)
    if h >= 3:
        assert not np.array_equal(I.field_metrics(frames, w, h, before, 0), I.field_metrics(frames, w, h, before, 8))


# ---- the standalone pass -------------------------------------------------------------------------------------------------------
def telecined(w, h, fmt, tff, phase, nfilm=8, seed=0x1F):
    film = I.film_frames(w, h, fmt, nfilm, seed + phase)
    clip, seq = I.telecine(film, w, h, fmt, tff, phase)
    return film, clip


def check_clip(pkg, clip, w, h, fmt, tff, nt=0, state=None):
    want = I.ivtc_clip(clip, w, h, fmt, tff, nt, state)
    got = pkg.ivtc_clip(clip, w, h, fmt, pkg.Ivtc(tff, nt), state=state)
    assert np.array_equal(got[1], want[1]), "match %s, not %s" % (got[1], want[1])
    assert np.array_equal(got[2], want[2]), "drop %s, not %s (D %s)" % (got[2], want[2], want[4])
    A.assert_same("pictures", got[0], want[0])
    A.assert_same("state", got[3], want[3])
    return want


@pytest.mark.parametrize("w,h,fmt", [(352, 288, A.SUBSAMP_420), (35, 19, A.SUBSAMP_444)])
def test_ivtc_clip_equals_numpy_and_the_film(pkg, mem, w, h, fmt):
    fb = A.frame_bytes(w, h, fmt)
    for tff in (1, 0):
        for phase in range(4):
            film, clip = telecined(w, h, fmt, tff, phase)
            assert clip.shape[0] == 10
            out, match, drop, state, _ = check_clip(pkg, clip, w, h, fmt, tff)
            # the feature itself, whatever the model says: the film frames come back
            got = pkg.ivtc_clip(clip, w, h, fmt, pkg.Ivtc(tff, 0))[0]
            assert got.shape == film.shape and np.array_equal(got, film), (tff, phase)
            assert (match == I.P).any() and (match == I.C).any()
            # two calls of 5 with the state passed on equal one call of 10
            a = pkg.ivtc_clip(clip[:5], w, h, fmt, pkg.Ivtc(tff, 0))
            b = pkg.ivtc_clip(clip[5:], w, h, fmt, pkg.Ivtc(tff, 0), state=a[3])
            assert np.array_equal(np.concatenate([a[0], b[0]]), out) and np.array_equal(np.concatenate([a[1], b[1]]), match)
            assert np.array_equal(np.concatenate([a[2], b[2]]), drop) and np.array_equal(b[3], state)
    # streams that start inside the pulldown cycle: the first picture stays combed, and from the third frame of the cycle on the
    # duplicate is a cycle's LAST picture -- the state's woven luma is one that was dropped
    film = I.film_frames(w, h, fmt, 16, 0x2A)
    full, _ = I.telecine(film, w, h, fmt, 1, 0)
    for lead in (2, 3):
        clip = full[lead:lead + 10]
        want = check_clip(pkg, clip, w, h, fmt, 1)
        first = check_clip(pkg, clip[:5], w, h, fmt, 1)
        check_clip(pkg, clip[5:], w, h, fmt, 1, state=first[3])
    assert list(I.ivtc_clip(full[3:13], w, h, fmt, 1)[2]) == [4, 4]
    # device memory: the buffers exactly as long as their contents inside larger allocations of a known pattern, aligned and not
    film, clip = telecined(w, h, fmt, 0, 1)
    st = I.ivtc_clip(clip[:5], w, h, fmt, 0)[3]
    want = I.ivtc_clip(clip[5:], w, h, fmt, 0, state=st)
    n, sb = 5, I.state_bytes(w, h, fmt)
    for off, doff in ((4096, 4096), (4096 + 3, 4096 + 16)):
        big_s = np.full(off + n * fb + 4096, 0xC3, dtype=np.uint8)
        big_s[off:off + n * fb] = clip[5:].reshape(-1)
        big_i = np.full(off + sb + 4096, 0x5A, dtype=np.uint8)
        big_i[off:off + sb] = st
        big_d = np.full(doff + 4 * fb + 4096, 0x3C, dtype=np.uint8)
        big_o = np.full(doff + sb + 4096, 0x3C, dtype=np.uint8)
        ps, pi, pd, po = (mem.alloc(x) for x in (big_s, big_i, big_d, big_o))
        _, match, drop = pkg.ivtc_clip(C.c_void_p(ps.value + off), w, h, fmt, pkg.Ivtc(0, 0), state=C.c_void_p(pi.value + off), n=n,
                                       out=C.c_void_p(pd.value + doff), state_out=C.c_void_p(po.value + doff))
        assert np.array_equal(match, want[1]) and np.array_equal(drop, want[2])
        after, safter = mem.read(pd, big_d.size), mem.read(po, big_o.size)
        assert (after[:doff] == 0x3C).all() and (after[doff + 4 * fb:] == 0x3C).all(), "written outside the destination"
        assert (safter[:doff] == 0x3C).all() and (safter[doff + sb:] == 0x3C).all(), "written outside the state"
        A.assert_same("device pictures, offsets %d %d" % (off, doff), after[doff:doff + 4 * fb].reshape(4, fb), want[0])
        A.assert_same("device state, offsets %d %d" % (off, doff), safter[doff:doff + sb], want[3])
        assert np.array_equal(mem.read(ps, big_s.size), big_s) and np.array_equal(mem.read(pi, big_i.size), big_i)
        # the state written over the state read
        pkg.ivtc_clip(C.c_void_p(ps.value + off), w, h, fmt, pkg.Ivtc(0, 0), state=C.c_void_p(pi.value + off), n=n,
                      out=C.c_void_p(pd.value + doff), state_out=C.c_void_p(pi.value + off))
        A.assert_same("state in place", mem.read(pi, big_i.size)[off:off + sb], want[3])
        A.assert_same("pictures, state in place", mem.read(pd, big_d.size)[doff:doff + 4 * fb].reshape(4, fb), want[0])


def test_static_clip(pkg):
    """every match C; D is 0 but for the stream's first picture (UINT32_MAX, never dropped unless all five tie), so a stream's first
    cycle drops picture 1 and every later cycle -- and the first cycle of a call that brings a state -- picture 0"""
    w, h, fmt = 35, 19, A.SUBSAMP_420
    one = I.film_frames(w, h, fmt, 1, 3)
    clip = np.repeat(one, 10, axis=0)
    out, match, drop, state = pkg.ivtc_clip(clip, w, h, fmt, pkg.Ivtc(1, 0))
    assert not match.any() and list(drop) == [1, 0] and np.array_equal(out, np.repeat(one, 8, axis=0))
    out, match, drop, _ = pkg.ivtc_clip(clip, w, h, fmt, pkg.Ivtc(0, 0), state=state)
    assert not match.any() and list(drop) == [0, 0] and np.array_equal(out, np.repeat(one, 8, axis=0))
    check_clip(pkg, clip, w, h, fmt, 1)


def test_noise_threshold(pkg):
    """one noisy clip on which nt = 0 and nt = 8 give different tables in numpy: the GPU gives both"""
    w, h, fmt = 352, 288, A.SUBSAMP_420
    film, clip = telecined(w, h, fmt, 1, 0)
    noisy = I.add_noise(clip, 0xBEE)
    a = check_clip(pkg, noisy, w, h, fmt, 1, nt=0)
    b = check_clip(pkg, noisy, w, h, fmt, 1, nt=8)
    assert not (np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]))


# ---- field order ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("speed", (1, 2))
def test_field_order(pkg, mem, speed):
    w, h, fmt = 64, 48, A.SUBSAMP_420
    for tff in (1, 0):
        clip = I.interlaced_pan(w, h, fmt, 20, 0x77, tff, speed)
        assert pkg.detect_field_order_clip(clip, w, h, fmt) == tff
        met = pkg.field_metrics_clip(clip, w, h, fmt)
        assert np.array_equal(met, I.field_metrics(clip, w, h)) and pkg.field_order_from_metrics(met) == tff
        assert pkg.detect_field_order_clip(mem.alloc(clip), w, h, fmt, n=20) == tff
        noisy = I.add_noise(clip, 0x78)
        assert pkg.detect_field_order_clip(noisy, w, h, fmt, nt=8) == tff
    still = I.static_columns(w, h, fmt, 20, 9)          # (tests/_ivtc.py says why a static clip for this has no vertical detail)
    assert pkg.detect_field_order_clip(still, w, h, fmt) == -1 and not pkg.field_metrics_clip(still, w, h, fmt).any()


# ---- sessions ------------------------------------------------------------------------------------------------------------------
_cache = {}


def sources(fmt, w=W, h=H):
    """S telecined sources of NCALLS calls (either phase parity), their film frames -- which the numpy pass gives back"""
    key = ("src", fmt, w, h)
    if key not in _cache:
        films, clips = [], []
        for s in range(S):
            film = I.film_frames(w, h, fmt, NCALLS * F, 0x3E0 + s)
            clip, _ = I.telecine(film, w, h, fmt, 1, s)
            assert np.array_equal(I.ivtc_clip(clip, w, h, fmt, 1)[0], film)
            films.append(film)
            clips.append(clip)
        _cache[key] = clips, films
    return _cache[key]


def oracle(key, clip, w, h, fmt, **rate):
    """the stream the oracle makes of a clip, once per key"""
    if key not in _cache:
        _cache[key] = A.orc_encode(clip, A.orc_cfg(w, h, fmt, **dict(CRF, **rate)), eos=False)[0]
    return _cache[key]


def calls_of(clips, per_call):
    """[S, frames of a call, bytes] per call"""
    return [np.ascontiguousarray(np.stack([c[k * per_call:(k + 1) * per_call] for c in clips])) for k in range(clips[0].shape[0] // per_call)]


def run(b, calls, form, pipelined=True):
    """submit / collect the calls -> streams"""
    dev = form != "host"
    junk = np.full(calls[0].size, 0xA5, dtype=np.uint8)
    ins = [b.upload(c) for c in calls] if dev else calls
    got = [b""] * b.nstreams

    def submit(c):
        b.submit(c, on_device=dev, held=form == "held")
        if form == "device":                             # a plain device clip is the caller's again when submit returns
            assert b.L.dsvg_dev_upload(b.ctx, c, junk.ctypes.data, junk.nbytes) == 0

    def take():
        got[:] = [x + bytes(p) for x, p in zip(got, b.collect())]

    if pipelined:
        submit(ins[0])
        for c in ins[1:]:
            submit(c)
            take()
        take()
    else:
        for c in ins:
            submit(c)
            take()
    return got


def test_batch(pkg, orc):
    fmt = A.SUBSAMP_420
    clips, films = sources(fmt)
    want = [oracle(("b", s), films[s], W, H, fmt, qp=80) for s in range(S)]
    calls = calls_of(clips, 5 * F // 4)
    assert len(calls) == NCALLS
    cfg = pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80))
    for form in ("host", "device", "held"):
        b = pkg.Batch(cfg, S, F)
        try:
            b.set_source_ivtc(pkg.Ivtc(1, 0))
            assert b.in_frames == 10
            got = run(b, calls, form, pipelined=form != "device")
        finally:
            b.close()
        for s in range(S):
            assert got[s] == want[s], "%s: source %d: not the oracle's stream of the film frames" % (form, s)


def test_reset_makes_the_next_picture_a_first_picture(pkg, orc):
    fmt = A.SUBSAMP_420
    # both sources start inside the pulldown cycle, so that a call's first frame needs the frame before it; source 1 is cut between
    # the calls, source 0 runs on
    clips = []
    for s in range(S):
        film = I.film_frames(W, H, fmt, 20, 0x4E0 + s)
        clips.append(I.telecine(film, W, H, fmt, 1, 0)[0][2:22])
    whole = [I.ivtc_clip(c, W, H, fmt, 1)[0] for c in clips]
    cut = np.concatenate([I.ivtc_clip(clips[1][:10], W, H, fmt, 1)[0], I.ivtc_clip(clips[1][10:], W, H, fmt, 1)[0]])
    assert not np.array_equal(cut, whole[1])
    want = [oracle(("reset", 0), whole[0], W, H, fmt, qp=80), oracle(("reset", 1), cut, W, H, fmt, qp=80)]
    calls = calls_of(clips, 10)
    b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
    try:
        b.set_source_ivtc(pkg.Ivtc(1, 0))
        first = b.encode(calls[0])
        b.ivtc_reset(1)
        second = b.encode(calls[1])
    finally:
        b.close()
    for s in range(S):
        assert bytes(first[s]) + bytes(second[s]) == want[s], s


def test_quality_ladder_and_chain_mode(pkg, orc):
    fmt = A.SUBSAMP_420
    qps = (60, 90)
    clips, films = sources(fmt)
    calls = calls_of(clips, 10)
    rungs = [pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=q)) for q in qps]
    for form in ("host", "held"):
        b = pkg.Ladder(rungs, S, F)
        try:
            b.set_source_ivtc(pkg.Ivtc(1, 0))
            got = run(b, calls, form)
        finally:
            b.close()
        for s in range(S):
            for r, q in enumerate(qps):
                assert got[s * 2 + r] == oracle(("l", s, q), films[s], W, H, fmt, qp=q), (form, s, r)
    # chain mode: one stream, consecutive frames
    want = oracle(("c",), films[0], W, H, fmt, qp=75)
    cfg = pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=75))
    for form in ("host", "device"):
        b = pkg.Batch(cfg, 1, F, chains=2)
        try:
            b.set_source_ivtc(pkg.Ivtc(1, 0))
            got = run(b, [c[:1] for c in calls], form, pipelined=False)
        finally:
            b.close()
        assert got[0] == want, form


def test_behind_a_uyvy_source(pkg, orc):
    """the converter's clips hold the 10 frames a call brings, not frames_per_call: whichever of the two is set first, and again after
    the pass is cleared and set"""
    fmt = A.SUBSAMP_422
    clips, films = sources(fmt)
    f = PF.pf(PF.UYVY)
    raws = [PF.pack(c.astype(np.uint32), f, W, H, fmt, np.random.default_rng(s)).reshape(c.shape[0], -1) for s, c in enumerate(clips)]
    for r, c in zip(raws, clips):
        assert np.array_equal(PF.convert(r.reshape(-1), f, W, H, fmt, c.shape[0]), c)
    want = [oracle(("u", s), films[s], W, H, fmt, qp=80) for s in range(S)]
    calls = calls_of(raws, 10)
    pf = pkg.PixFormat(f["layout"], f["depth"], f["msb"], f["pitch"], f["frame_bytes"])
    for order in ("format first", "ivtc first", "cleared and set again"):
        b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
        try:
            if order == "ivtc first":
                b.set_source_ivtc(pkg.Ivtc(1, 0))
                b.set_source_format(pf)
            else:
                b.set_source_format(pf)
                b.set_source_ivtc(pkg.Ivtc(1, 0))
            if order == "cleared and set again":
                b.set_source_ivtc(None)
                assert b.in_frames == F
                plain = b.encode(calls_of(raws, F)[0])
                assert bytes(plain[0]) == oracle(("u plain",), clips[0][:F], W, H, fmt, qp=80)
                b.close()
                b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
                b.set_source_format(pf)
                b.set_source_ivtc(pkg.Ivtc(0, 3))
                b.set_source_ivtc(None)
                b.set_source_ivtc(pkg.Ivtc(1, 0))
            got = run(b, calls, "host" if order == "ivtc first" else "device")
        finally:
            b.close()
        assert got == want, order


def test_in_front_of_the_noise_filter_and_the_reframe(pkg, orc):
    fmt = A.SUBSAMP_420
    IW, IH = 80, 56
    RF = R.rf(IW, IH, (8, 4, W, H - 8), (W, H), (0, 4))
    dn = (24, 16)
    clips, films = sources(fmt, IW, IH)
    want = []
    for s in range(S):
        filtered = DN.denoise_clip(films[s], IW, IH, fmt, *dn)[0]
        want.append(oracle(("dnrf", s), R.reframe_clip(filtered, RF, fmt), W, H, fmt, qp=80))
    calls = calls_of(clips, 10)
    b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
    try:
        b.set_source_reframe(pkg.Reframe(IW, IH, (RF["x"], RF["y"], RF["w"], RF["h"]), (W, H), (RF["dst_x"], RF["dst_y"]), RF["fill"]))
        b.set_source_denoise(pkg.Denoise(*dn))
        b.set_source_ivtc(pkg.Ivtc(1, 0))
        got = run(b, calls, "host")
    finally:
        b.close()
    assert got == want


def test_resolution_ladder(pkg, orc):
    fmt = A.SUBSAMP_420
    LW, LH = 128, 96
    geoms = [(LW, LH, 80), (W, H, 70)]
    clips, films = sources(fmt, LW, LH)
    want = []
    for s, film in enumerate(films):
        for gw, gh, qp in geoms:
            sc = film if (gw, gh) == (LW, LH) else Z.scale_clip(film, LW, LH, fmt, gw, gh, Z.CUBIC)
            want.append(oracle(("r", s, gw), sc, gw, gh, fmt, qp=qp))
    for form in ("host", "device"):
        b = pkg.ResLadder(LW, LH, fmt, [(gw, gh, [pkg.make_encoder_cfg(gw, gh, fmt, **dict(CRF, qp=qp))]) for gw, gh, qp in geoms], S, F, Z.CUBIC)
        try:
            b.set_ivtc(pkg.Ivtc(1, 0))
            assert b.in_frames == 10
            calls = calls_of(clips, b.in_frames)
            dev = form != "host"
            ins = [b.upload(c) for c in calls] if dev else calls
            got = [b""] * b.nstreams
            for c in ins[:2]:
                b.submit(c, on_device=dev)
            got[:] = [x + bytes(p) for x, p in zip(got, b.collect())]
            b.submit(ins[2], on_device=dev)
            for _ in range(2):
                got[:] = [x + bytes(p) for x, p in zip(got, b.collect())]
        finally:
            b.close()
        for k, data in enumerate(want):
            assert got[k] == data, "%s: output stream %d: packets differ from the oracle's" % (form, k)


def test_error_contract(pkg, orc):
    """every DSVG_ERR_ARG leaves the setting, and the state, as they were"""
    fmt = A.SUBSAMP_420
    L = pkg.lib()
    clips, films = sources(fmt)
    want = oracle(("b", 0), films[0], W, H, fmt, qp=80)
    cfg = pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80))
    calls = calls_of(clips[:1], 10)
    iv = pkg.Ivtc(1, 0)
    six = pkg.Batch(cfg, 1, 6)
    b = pkg.Batch(cfg, 1, F)
    r = pkg.ResLadder(W, H, fmt, [(W, H, [pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=70))])], 1, 6, Z.CUBIC)
    try:
        assert L.dsv1_batch_set_source_ivtc(six.h, C.byref(iv)) == DSVG_ERR_ARG                                # frames_per_call % 4
        assert not L.dsv1_batch_has_source_lane(six.h)
        assert L.dsv1_resladder_set_ivtc(r.h, C.byref(iv)) == DSVG_ERR_ARG
        assert L.dsv1_resladder_ivtc_reset(r.h, -1) == DSVG_ERR_ARG                                            # none set
        assert L.dsv1_batch_ivtc_reset(b.h, -1) == DSVG_ERR_ARG
        bads = []
        for tff, nt, res in ((2, 0, 0), (-1, 0, 0), (1, -1, 0), (1, 255, 0), (1, 0, 1)):
            x = pkg.Ivtc(1, 0)
            x.tff, x.nt, x.reserved[1] = tff, nt, res
            bads.append(x)
        for bad in bads:
            assert L.dsv1_batch_set_source_ivtc(b.h, C.byref(bad)) == DSVG_ERR_ARG
        assert not L.dsv1_batch_has_source_lane(b.h)
        # exclusive with the deinterlacer, either way round
        b.set_source_deinterlace(pkg.Deint(0, 1))
        assert L.dsv1_batch_set_source_ivtc(b.h, C.byref(iv)) == DSVG_ERR_ARG
        assert L.dsv1_batch_ivtc_reset(b.h, -1) == DSVG_ERR_ARG
        b.deinterlace_reset(-1)                           # (the deinterlacer is still the one set)
        b.set_source_deinterlace(None)
        b.set_source_ivtc(iv)
        assert L.dsv1_batch_set_source_deinterlace(b.h, C.byref(pkg.Deint(0, 1))) == DSVG_ERR_ARG
        assert L.dsv1_batch_deinterlace_reset(b.h, -1) == DSVG_ERR_ARG
        for bad in bads:
            assert L.dsv1_batch_set_source_ivtc(b.h, C.byref(bad)) == DSVG_ERR_ARG
        assert L.dsv1_batch_ivtc_reset(b.h, 1) == DSVG_ERR_ARG and L.dsv1_batch_ivtc_reset(b.h, -2) == DSVG_ERR_ARG
        # a reframe is set before the other passes, never behind them
        good = pkg.Reframe(80, 56, (8, 4, W, H), (W, H))
        assert L.dsv1_batch_set_source_reframe(b.h, C.byref(good)) == DSVG_ERR_ARG
        pin = b.pinned(calls[0].shape)
        pin[...] = calls[0]
        assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == DSVG_ERR_ARG
        with pytest.raises(ValueError):
            b.submit(calls[0][:, :F])
        b.submit(pin)
        assert L.dsv1_batch_set_source_ivtc(b.h, None) == DSVG_ERR_ARG                                         # a batch in flight
        assert L.dsv1_batch_set_source_ivtc(b.h, C.byref(pkg.Ivtc(0, 8))) == DSVG_ERR_ARG
        assert L.dsv1_batch_ivtc_reset(b.h, 0) == DSVG_ERR_ARG
        first = bytes(b.collect()[0])
        # every refusal left the setting, and the state, as they were: the stream goes on as the uncut clip's
        rest = b"".join(bytes(b.encode(c)[0]) for c in calls[1:])
        assert first + rest == want
        b.set_source_ivtc(None)
        assert not L.dsv1_batch_has_source_lane(b.h)
    finally:
        six.close()
        b.close()
        r.close()
