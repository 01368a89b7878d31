"""The levels pass and the histogram on the GPU (include/dsv1_api.h, Levels; csrc/k_levels.hip): dsv1_levels_clip equals the numpy
statement tests/_levels.py, in place too, touching nothing around its buffers; dsv1_histogram_clip equals np.bincount; batches, quality
ladders, chain mode and resolution ladders with levels set write the packets of the same session fed the numpy-levelled clip, which are
the oracle's streams of it."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import _chroma as CH
import _deint as DI
import _denoise as D
import _ivtc as I
import _levels as LV
import _orient as O
import _pixfmt as PF
import _reframe as R
import _rgb as RG
import _scale as Z

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2
CRF = dict(gop=4, rc_mode_cli=1, scd=1)
S, F = 2, 4
W, H = 70, 50                                             # the sessions' geometry
GUARD = 64
T_RANGE = LV.range_(1, 0)                                 # full range -> limited
T_GRADE = LV.compose(LV.range_(1, 0), LV.adjust(24, 228, 16, 235, 300))
T_OTHER = LV.adjust(8, 200, 0, 255, 128)


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


def lv_of(pkg, t):
    return pkg.Levels.from_tables(t)


# ---- the standalone calls --------------------------------------------------------------------------------------------------------
def table_sets(seed):
    rnd = LV.random_tables(seed)
    one_identity = LV.random_tables(seed + 1)
    one_identity[seed % 3] = np.arange(256)
    constant = np.repeat(np.array([[7], [200], [131]], dtype=np.uint8), 256, axis=1)
    return [("random", rnd), ("one identity", one_identity), ("constant", constant)]


def check_levels(pkg, mem, fmt, w, h, n, name, t):
    fb = A.frame_bytes(w, h, fmt)
    src = LV.noise(n, w, h, fmt, 0x1E0 + fmt + w)
    want = LV.levels_clip(src, w, h, fmt, t)
    lv = lv_of(pkg, t)
    tag = "%s 0x%x %dx%d n=%d" % (name, fmt, w, h, n)
    # host memory: the output between 64 sentinel bytes on each side
    big = np.full(2 * GUARD + want.size, 0xC3, dtype=np.uint8)
    out = big[GUARD:GUARD + want.size]
    pkg.levels_clip(src, w, h, fmt, lv, out=out)
    assert (big[:GUARD] == 0xC3).all() and (big[GUARD + want.size:] == 0xC3).all(), "written outside the destination (host) " + tag
    A.assert_same("host " + tag, out.reshape(want.shape), want)
    # host memory, in place
    big[GUARD:GUARD + want.size] = src.reshape(-1)
    pkg.levels_clip(out, w, h, fmt, lv, out=out)
    assert (big[:GUARD] == 0xC3).all() and (big[GUARD + want.size:] == 0xC3).all(), "written outside the destination (host, in place) " + tag
    A.assert_same("host in place " + tag, out.reshape(want.shape), want)
    # device memory: source and destination exactly as long as their contents, at two alignments each
    for soff, doff in ((256, GUARD), (256 + 3, GUARD + 5)):
        big_s = np.full(soff + n * fb + 64, 0x99, dtype=np.uint8)
        big_s[soff:soff + n * fb] = src.reshape(-1)
        big_d = np.full(doff + want.size + GUARD, 0x3C, dtype=np.uint8)
        ps, pd = mem.alloc(big_s), mem.alloc(big_d)
        pkg.levels_clip(C.c_void_p(ps.value + soff), w, h, fmt, lv, n=n, out=C.c_void_p(pd.value + doff))
        after = mem.read(pd, big_d.size)
        assert (after[:doff] == 0x3C).all() and (after[doff + want.size:] == 0x3C).all(), "written outside the destination (device) " + tag
        A.assert_same("device offsets %d %d %s" % (soff, doff, tag), after[doff:doff + want.size].reshape(want.shape), want)
        assert np.array_equal(mem.read(ps, big_s.size), big_s)
        # dst == src: the clip between its guards, levelled where it lies
        p = C.c_void_p(ps.value + soff)
        pkg.levels_clip(p, w, h, fmt, lv, n=n, out=p)
        after = mem.read(ps, big_s.size)
        assert (after[:soff] == 0x99).all() and (after[soff + n * fb:] == 0x99).all(), "written outside the clip (device, in place) " + tag
        A.assert_same("device in place %d %s" % (soff, tag), after[soff:soff + n * fb].reshape(want.shape), want)


@pytest.mark.parametrize("fmt", LV.FORMATS, ids=["0x%x" % f for f in LV.FORMATS])
def test_levels_clip_equals_numpy(pkg, mem, fmt):
    assert A.frame_bytes(17, 3, A.SUBSAMP_420) == 87
    for k, (w, h) in enumerate(LV.SMALL):
        for n in (1, 3):
            for name, t in table_sets(0x70 + 3 * k + n):
                check_levels(pkg, mem, fmt, w, h, n, name, t)


@pytest.mark.parametrize("n", [1, 3])
def test_levels_clip_equals_numpy_1080p(pkg, mem, n):
    check_levels(pkg, mem, A.SUBSAMP_420, *LV.BIG, n, *table_sets(0x90 + n)[0])


def test_levels_clip_builders_end_to_end(pkg):
    """the Python builders are the library's: a full-range ramp comes out limited"""
    fmt, w, h = A.SUBSAMP_444, 16, 16
    ramp = np.tile(np.arange(256, dtype=np.uint8), 3)[None]
    out = pkg.levels_clip(ramp, w, h, fmt, pkg.Levels.range(1, 0))
    assert np.array_equal(out, LV.levels_clip(ramp, w, h, fmt, T_RANGE))
    assert (out[0, 0], out[0, 255], out[0, 256], out[0, 511]) == (16, 235, 16, 240)
    assert np.array_equal(pkg.Levels.range(1, 0).compose(pkg.Levels.adjust(24, 228, 16, 235, 300)).tables(), T_GRADE)
    assert pkg.Levels.identity().is_identity() and not pkg.Levels.range(0, 1).is_identity()
    assert np.array_equal(pkg.levels_clip(ramp, w, h, fmt, pkg.Levels.identity()), ramp)          # the identity still copies


def hist_clips(n, w, h, fmt, seed):
    fb = A.frame_bytes(w, h, fmt)
    ramp = ((np.arange(n * fb, dtype=np.int64) + 37 * (np.arange(n * fb) // fb)) % 256).astype(np.uint8).reshape(n, fb)
    return [("random", LV.noise(n, w, h, fmt, seed)), ("flat", np.full((n, fb), 16 + seed % 200, dtype=np.uint8)), ("each value once per row", ramp)]


def check_histogram(pkg, mem, fmt, w, h, n):
    cw, ch = A.chroma_dims(w, h, fmt)
    for name, clip in hist_clips(n, w, h, fmt, 0x2A0 + w + fmt):
        tag = "%s 0x%x %dx%d n=%d" % (name, fmt, w, h, n)
        want = LV.histogram(clip, w, h, fmt)
        got = pkg.histogram_clip(clip, w, h, fmt)
        assert got.dtype == np.uint32 and got.shape == (n, 3, 256)
        A.assert_same("host " + tag, got, want)
        assert (got.sum(axis=2, dtype=np.uint64) == np.array([w * h, cw * ch, cw * ch], dtype=np.uint64)).all(), tag
        big = np.full(256 + 3 + clip.size + 64, 0x99, dtype=np.uint8)
        for off in (256, 256 + 3):
            big[:] = 0x99
            big[off:off + clip.size] = clip.reshape(-1)
            p = mem.alloc(big)
            A.assert_same("device offset %d %s" % (off, tag), pkg.histogram_clip(C.c_void_p(p.value + off), w, h, fmt, n=n), want)
        for ppm in (0, 1000, 999999):
            two_step = pkg.range_from_histogram(got, ppm)
            assert two_step == LV.range_from_histogram(want, ppm)
            assert pkg.detect_range_clip(clip, w, h, fmt, ppm=ppm) == two_step, (tag, ppm)


@pytest.mark.parametrize("fmt", LV.FORMATS, ids=["0x%x" % f for f in LV.FORMATS])
def test_histogram_clip_equals_bincount(pkg, mem, fmt):
    for w, h in LV.SMALL:
        for n in (1, 3):
            check_histogram(pkg, mem, fmt, w, h, n)


def test_histogram_clip_equals_bincount_1080p(pkg, mem):
    check_histogram(pkg, mem, A.SUBSAMP_420, *LV.BIG, 2)


def test_detect_range_tells_a_full_range_clip_from_a_limited_one(pkg):
    fmt = A.SUBSAMP_420
    full = A.gen_clip(W, H, fmt, 0x4E0, 2, style=1)
    full[:, ::7] = 0
    full[:, 3::7] = 255
    limited = LV.levels_clip(full, W, H, fmt, T_RANGE)
    assert pkg.detect_range_clip(full, W, H, fmt) is True and pkg.detect_range_clip(limited, W, H, fmt) is False
    assert pkg.points_from_histogram(pkg.histogram_clip(limited, W, H, fmt), 0, 0) == (16, 235)
    assert pkg.points_from_histogram(pkg.histogram_clip(full, W, H, fmt), 0, 0) == (0, 255)


# ---- sessions ------------------------------------------------------------------------------------------------------------------
_cache = {}


def sources(fmt, w, h, n=2 * F):
    key = ("src", fmt, w, h, n)
    if key not in _cache:
        _cache[key] = [A.gen_clip(w, h, fmt, 0x4E0 + s, n, style=s & 1) for s in range(S)]
    return _cache[key]


def oracle(key, clip, w, h, fmt, **rate):
    if key not in _cache:
        _cache[key] = A.orc_encode(clip, A.orc_cfg(w, h, fmt, **dict(CRF, **rate)), want_recon=True, eos=False)
    return _cache[key]


def calls_of(clips, per_call):
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


def fed(make, clips, form="host", pipelined=True):
    """the packets of the same session fed the numpy-levelled clips, nothing set"""
    b = make()
    try:
        return run(b, calls_of(clips, F), form, pipelined)
    finally:
        b.close()


def test_plain_batch(pkg, orc):
    fmt = A.SUBSAMP_420
    clips = sources(fmt, W, H)
    lev = [LV.levels_clip(c, W, H, fmt, T_GRADE) for c in clips]
    want = [oracle(("b", s), lev[s], W, H, fmt, qp=80)[0] for s in range(S)]
    assert want[0] != oracle(("off", 0), clips[0], W, H, fmt, qp=80)[0]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
    assert fed(make, lev) == want
    calls = calls_of(clips, F)
    assert len(calls) == 2
    for form, pipelined in (("host", True), ("host", False), ("device", False), ("held", True)):
        b = make()
        try:
            b.set_source_levels(lv_of(pkg, T_GRADE))
            assert b.L.dsv1_batch_has_source_lane(b.h)
            got = run(b, calls, form, pipelined)
        finally:
            b.close()
        assert got == want, (form, pipelined)


def test_quality_ladder_and_chain_mode(pkg, orc):
    fmt = A.SUBSAMP_420
    qps = (60, 90)
    clips = sources(fmt, W, H)
    lev = [LV.levels_clip(c, W, H, fmt, T_RANGE) for c in clips]
    calls = calls_of(clips, F)
    rungs = [pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=q)) for q in qps]
    want = [oracle(("l", s, q), lev[s], W, H, fmt, qp=q)[0] for s in range(S) for q in qps]
    assert fed(lambda: pkg.Ladder(rungs, S, F), lev) == want
    for form in ("host", "held"):
        b = pkg.Ladder(rungs, S, F)
        try:
            b.set_source_levels(pkg.Levels.range(1, 0))
            got = run(b, calls, form)
        finally:
            b.close()
        assert got == want, form
    want = oracle(("c",), lev[0], W, H, fmt, qp=75)[0]
    cfg = pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=75))
    for form in ("host", "device"):
        b = pkg.Batch(cfg, 1, F, chains=2)
        try:
            b.set_source_levels(pkg.Levels.range(1, 0))
            got = run(b, [c[:1] for c in calls], form, pipelined=False)
        finally:
            b.close()
        assert got[0] == want, form


def cpf(pkg, f):
    return pkg.PixFormat(f["layout"], f["depth"], f["msb"], f["pitch"], f["frame_bytes"])


def test_behind_a_uyvy_422_source_halved_to_420(pkg, orc):
    fmt, sfmt = A.SUBSAMP_420, A.SUBSAMP_422
    f = PF.pf(PF.UYVY)
    planar = sources(sfmt, W, H)
    raws = [PF.pack(c.astype(np.uint32), f, W, H, sfmt, np.random.default_rng(s)).reshape(c.shape[0], -1) for s, c in enumerate(planar)]
    lev = [LV.levels_clip(CH.convert_sub(r.reshape(-1), f, W, H, sfmt, fmt, r.shape[0]), W, H, fmt, T_GRADE) for r in raws]
    want = [oracle(("u", s), lev[s], W, H, fmt, qp=80)[0] for s in range(S)]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
    assert fed(make, lev) == want
    for form, first in (("host", "levels"), ("device", "format")):
        b = make()
        try:
            if first == "levels":
                b.set_source_levels(lv_of(pkg, T_GRADE))
            b.set_source_format(cpf(pkg, f), src_subsamp=sfmt)
            if first == "format":
                b.set_source_levels(lv_of(pkg, T_GRADE))
            assert b.frame_bytes == raws[0].shape[1]
            got = run(b, calls_of(raws, F), form)
        finally:
            b.close()
        assert got == want, form


def test_behind_an_rgb_source(pkg, orc):
    fmt, n = A.SUBSAMP_420, 2 * F
    f = RG.rf(RG.BGRA, RG.BT709, 1)                      # the import matrix writes full-range YCbCr; the levels bring it to limited
    raws, lev = [], []
    for s in range(S):
        rgb = A.gen_clip(W, H, A.SUBSAMP_444, 0x5C0 + s, n, style=1)
        Rr, G, B = (rgb[:, k * W * H:(k + 1) * W * H].reshape(n, H, W) for k in range(3))
        raw = RG.pack(Rr, G, B, f, W, H, np.random.default_rng(s))
        raws.append(raw.reshape(n, -1))
        lev.append(LV.levels_clip(RG.import_(raw, f, W, H, fmt, n), W, H, fmt, T_RANGE))
    want = [oracle(("rgb", s), lev[s], W, H, fmt, qp=80)[0] for s in range(S)]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
    assert fed(make, lev) == want
    for form in ("host", "held"):
        b = make()
        try:
            b.set_source_rgb(pkg.RgbFormat(f["order"], f["matrix"], f["full"], f["upsample"], f["pitch"], f["frame_bytes"]))
            b.set_source_levels(pkg.Levels.range(1, 0))
            got = run(b, calls_of(raws, F), form)
        finally:
            b.close()
        assert got == want, form


@pytest.mark.parametrize("mode", [DI.FRAME, DI.FIELD], ids=["frame-rate", "field-rate"])
def test_in_front_of_the_deinterlacer_and_the_noise_filter_across_two_calls(pkg, orc, mode):
    """levels -> deinterlacer -> noise filter, two calls: the passes behind the levels see the levelled pictures, and their history
    and state cross the call boundary"""
    fmt, dn = A.SUBSAMP_420, (24, 24)
    nin = F // 2 if mode == DI.FIELD else F               # input frames per call
    clips = [DI.gen_interlaced(W, H, fmt, 2 * nin, 0x1F0 + s, 1) for s in range(S)]
    lev = [LV.levels_clip(c, W, H, fmt, T_GRADE) for c in clips]
    den = [D.denoise_clip(DI.deint_clip(c, W, H, fmt, mode, 1), W, H, fmt, *dn)[0] for c in lev]
    cut = D.denoise_clip(DI.deint_clip(lev[0][nin:], W, H, fmt, mode, 1), W, H, fmt, *dn)[0]
    assert not np.array_equal(den[0][F:], cut)           # (the second call's history and state matter)
    want = [oracle(("di", mode, s), den[s], W, H, fmt, qp=80)[0] for s in range(S)]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
    assert fed(make, den) == want
    calls = calls_of(clips, nin)
    assert len(calls) == 2
    for form in ("host", "device"):
        b = make()
        try:
            b.set_source_deinterlace(pkg.Deint(mode, 1))
            b.set_source_levels(lv_of(pkg, T_GRADE))
            b.set_source_denoise(pkg.Denoise(*dn))
            got = run(b, calls, form, pipelined=form == "host")
        finally:
            b.close()
        assert got == want, form


def test_in_front_of_the_inverse_telecine(pkg, orc):
    """frames_per_call 4, so a call brings 5 frames: the levels' clips are allocated again with the converter's when the inverse
    telecine is installed (levels set before it) and are sized for 5 from the start (levels set after it); then the inverse telecine is
    cleared and the levels stay"""
    fmt, IW, IH = A.SUBSAMP_420, 64, 48
    films, clips = [], []
    for s in range(S):
        film = I.film_frames(IW, IH, fmt, 2 * F, 0x3E0 + s)
        clip, _ = I.telecine(film, IW, IH, fmt, 1, s)
        assert clip.shape[0] == 10
        films.append(film)
        clips.append(clip)
    lev = [LV.levels_clip(c, IW, IH, fmt, T_GRADE) for c in clips]
    back = []
    for c in lev:                                        # two calls of 5 frames, the state handed from the first to the second
        o1, _, _, state, _ = I.ivtc_clip(c[:5], IW, IH, fmt, 1)
        back.append(np.concatenate([o1, I.ivtc_clip(c[5:], IW, IH, fmt, 1, state=state)[0]]))
    assert back[0].shape[0] == 2 * F
    want = [oracle(("iv", s), back[s], IW, IH, fmt, qp=80)[0] for s in range(S)]
    plain = [oracle(("iv plain", s), lev[s][:F], IW, IH, fmt, qp=80)[0] for s in range(S)]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(IW, IH, fmt, **dict(CRF, qp=80)), S, F)
    assert fed(make, back) == want
    calls = calls_of(clips, 5)
    assert len(calls) == 2
    for order in ("levels first", "ivtc first"):
        b = make()
        try:
            if order == "levels first":
                b.set_source_levels(lv_of(pkg, T_GRADE))
                b.set_source_ivtc(pkg.Ivtc(1, 0))
            else:
                b.set_source_ivtc(pkg.Ivtc(1, 0))
                b.set_source_levels(lv_of(pkg, T_GRADE))
            assert b.in_frames == 5
            got = run(b, calls, "host" if order == "levels first" else "device")
        finally:
            b.close()
        assert got == want, order
        # ... and cleared: 4 frames a call again, the levels still applied
        b = make()
        try:
            if order == "levels first":
                b.set_source_levels(lv_of(pkg, T_GRADE))
                b.set_source_ivtc(pkg.Ivtc(1, 0))
            else:
                b.set_source_ivtc(pkg.Ivtc(1, 0))
                b.set_source_levels(lv_of(pkg, T_GRADE))
            b.set_source_ivtc(None)
            assert b.in_frames == F
            got = [bytes(p) for p in b.encode(calls_of([c[:F] for c in clips], F)[0])]
        finally:
            b.close()
        assert got == plain, order


RF = R.rf(W, H, (6, 4, 51, 33), (96, 64), (10, 8))        # the reframe test's window of the 70 x 50 picture on its 96 x 64 canvas


def test_with_orientation_and_reframe_set_before_it(pkg, orc):
    fmt, RW, RH = A.SUBSAMP_420, H, W                     # the raw clips are portrait
    clips = sources(fmt, RW, RH)
    lev = [LV.levels_clip(c, RW, RH, fmt, T_GRADE) for c in clips]
    framed = [R.reframe_clip(O.orient_clip(c, RW, RH, fmt, O.ROT90), RF, fmt) for c in lev]
    want = [oracle(("rf", s), framed[s], 96, 64, fmt, qp=80)[0] for s in range(S)]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(96, 64, fmt, **dict(CRF, qp=80)), S, F)
    assert fed(make, framed) == want
    for form in ("host", "device", "held"):
        b = make()
        try:
            b.set_source_reframe(pkg.Reframe(RF["in_w"], RF["in_h"], (RF["x"], RF["y"], RF["w"], RF["h"]), (96, 64), (RF["dst_x"], RF["dst_y"]), RF["fill"]))
            b.set_source_orient(O.ROT90)
            b.set_source_levels(lv_of(pkg, T_GRADE))     # LAST: it resolves at the raw geometry
            assert b.in_dims == (RW, RH) and b.frame_bytes == A.frame_bytes(RW, RH, fmt)
            got = run(b, calls_of(clips, F), form, pipelined=form != "device")
        finally:
            b.close()
        assert got == want, form


LW, LH = 128, 96


def ladder_run(b, calls, form):
    dev = form != "host"
    ins = [b.upload(c) for c in calls] if dev else calls
    got, xs, xp = [b""] * b.nstreams, [], []
    for c in ins:
        b.submit(c, on_device=dev, held=form == "held")
    for _ in ins:
        got[:] = [x + bytes(p) for x, p in zip(got, b.collect())]
        xs.append(b.src_sse())
        xp.append(b.src_psnr())
    return got, np.concatenate(xs, axis=1), np.concatenate(xp, axis=1)


def test_resolution_ladder(pkg, orc):
    fmt = A.SUBSAMP_420
    shapes = [(LW, LH, 80), (LW // 2, LH // 2, 70)]      # one geometry of the source's own size
    clips = sources(fmt, LW, LH)
    lev = [LV.levels_clip(c, LW, LH, fmt, T_GRADE) for c in clips]
    want = []
    for s, clip in enumerate(lev):
        for gw, gh, qp in shapes:
            sc = clip if (gw, gh) == (LW, LH) else Z.scale_clip(clip, LW, LH, fmt, gw, gh, Z.CUBIC)
            want.append(oracle(("r", s, gw), sc, gw, gh, fmt, qp=qp)[0])
    geoms = lambda: [(gw, gh, [pkg.make_encoder_cfg(gw, gh, fmt, **dict(CRF, qp=qp))]) for gw, gh, qp in shapes]
    # the ladder fed the levelled clip: packets and source-resolution figures to compare with
    b = pkg.ResLadder(LW, LH, fmt, geoms(), S, F, Z.CUBIC)
    try:
        b.src_quality_enable(sse=True, ssim=False, filt=Z.CUBIC)
        base, bsse, bpsnr = ladder_run(b, calls_of(lev, F), "host")
    finally:
        b.close()
    assert base == want
    # (measured against the clips as they came in, the figures would differ)
    b = pkg.ResLadder(LW, LH, fmt, geoms(), S, F, Z.CUBIC)
    try:
        b.src_quality_enable(sse=True, ssim=False, filt=Z.CUBIC)
        _, osse, _ = ladder_run(b, calls_of(clips, F), "host")
    finally:
        b.close()
    assert not np.array_equal(osse, bsse)
    for form in ("host", "held"):
        b = pkg.ResLadder(LW, LH, fmt, geoms(), S, F, Z.CUBIC)
        try:
            b.set_levels(lv_of(pkg, T_GRADE))
            b.src_quality_enable(sse=True, ssim=False, filt=Z.CUBIC)
            got, xsse, xpsnr = ladder_run(b, calls_of(clips, F), form)
        finally:
            b.close()
        assert got == want, form
        assert np.array_equal(xsse, bsse) and np.array_equal(xpsnr, bpsnr), form            # src_psnr() is against the LEVELLED source


def test_changing_the_tables_forgets_the_noise_filters_state(pkg, orc):
    fmt, dn = A.SUBSAMP_420, (24, 24)
    clips = sources(fmt, W, H)
    a = [LV.levels_clip(c[:F], W, H, fmt, T_GRADE) for c in clips]
    b2 = [LV.levels_clip(c[F:], W, H, fmt, T_OTHER) for c in clips]
    first = [D.denoise_clip(x, W, H, fmt, *dn) for x in a]
    fresh = [np.concatenate([first[s][0], D.denoise_clip(b2[s], W, H, fmt, *dn)[0]]) for s in range(S)]
    carried = np.concatenate([first[0][0], D.denoise_clip(b2[0], W, H, fmt, *dn, state=first[0][1])[0]])
    assert not np.array_equal(carried, fresh[0])         # (a filter that kept its state would show)
    want = [oracle(("forget", s), fresh[s], W, H, fmt, qp=80)[0] for s in range(S)]
    calls = calls_of(clips, F)
    b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
    try:
        b.set_source_denoise(pkg.Denoise(*dn))
        b.set_source_levels(lv_of(pkg, T_GRADE))
        p1 = b.encode(calls[0])
        b.set_source_levels(lv_of(pkg, T_OTHER))
        p2 = b.encode(calls[1])
    finally:
        b.close()
    assert [bytes(x) + bytes(y) for x, y in zip(p1, p2)] == want


# ---- errors and the feature off --------------------------------------------------------------------------------------------------
def test_error_contract(pkg, orc):
    fmt = A.SUBSAMP_420
    L = pkg.lib()
    clips = sources(fmt, W, H)[:1]
    lev = LV.levels_clip(clips[0], W, H, fmt, T_GRADE)
    want = oracle(("b", 0), lev, W, H, fmt, qp=80)[0]
    plain = oracle(("off", 0), clips[0], W, H, fmt, qp=80)[0]
    cfg = pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80))
    calls = calls_of(clips, F)
    setter = L.dsv1_batch_set_source_levels
    grade, other = lv_of(pkg, T_GRADE), lv_of(pkg, T_OTHER)
    b = pkg.Batch(cfg, 1, F)
    try:
        # NULL and the identity both clear the pass: no lane
        b.set_source_levels(grade)
        assert L.dsv1_batch_has_source_lane(b.h)
        b.set_source_levels(None)
        assert not L.dsv1_batch_has_source_lane(b.h)
        b.set_source_levels(grade)
        b.set_source_levels(pkg.Levels.identity())
        assert not L.dsv1_batch_has_source_lane(b.h)
        b.set_source_levels(pkg.Levels.range(1, 1))
        assert not L.dsv1_batch_has_source_lane(b.h)
        # a clip staged, a batch in flight: refused, and the batch codes the clips themselves
        pin = b.pinned(calls[0].shape)
        pin[...] = calls[0]
        assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == 0
        assert setter(b.h, C.byref(grade)) == DSVG_ERR_ARG
        b.submit(pin)
        assert setter(b.h, C.byref(grade)) == DSVG_ERR_ARG and setter(b.h, None) == DSVG_ERR_ARG
        p1 = bytes(b.collect()[0])
        assert not L.dsv1_batch_has_source_lane(b.h)
        assert p1 + bytes(b.encode(calls[1])[0]) == plain
        assert setter(None, C.byref(grade)) == DSVG_ERR_ARG
    finally:
        b.close()
    b = pkg.Batch(cfg, 1, F)
    try:
        b.set_source_levels(grade)
        pin = b.pinned(calls[0].shape)
        pin[...] = calls[0]
        assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == DSVG_ERR_ARG                                          # stage is refused while set
        onto = pkg.Reframe(80, 60, (4, 4, W, H), (W, H), (0, 0), RF["fill"])
        assert L.dsv1_reframe_valid(C.byref(onto), fmt)
        assert L.dsv1_batch_set_source_reframe(b.h, C.byref(onto)) == DSVG_ERR_ARG                               # a reframe comes BEFORE it
        assert L.dsv1_batch_set_source_reframe(b.h, None) == DSVG_ERR_ARG
        for code in (O.HFLIP, O.ROT90, O.NONE):
            assert L.dsv1_batch_set_source_orient(b.h, code) == DSVG_ERR_ARG                                     # ... and so does an orientation
        assert b.in_dims == (W, H)
        b.submit(pin)
        for x in (other, grade, pkg.Levels.identity()):                                                          # in flight: as it was
            assert setter(b.h, C.byref(x)) == DSVG_ERR_ARG
        assert setter(b.h, None) == DSVG_ERR_ARG
        first = b.collect()[0]
        assert bytes(first) + bytes(b.encode(calls[1])[0]) == want
        b.set_source_levels(None)                        # cleared: the reframe and the orientation may be set again
        assert L.dsv1_batch_set_source_orient(b.h, O.HFLIP) == 0 and L.dsv1_batch_set_source_orient(b.h, O.NONE) == 0
        assert not L.dsv1_batch_has_source_lane(b.h)
    finally:
        b.close()
    # the resolution ladder's setter
    r = pkg.ResLadder(LW, LH, fmt, [(LW, LH, [pkg.make_encoder_cfg(LW, LH, fmt, **dict(CRF, qp=80))])], 1, F, Z.CUBIC)
    try:
        assert L.dsv1_resladder_set_levels(None, C.byref(grade)) == DSVG_ERR_ARG
        r.set_levels(grade)
        r.submit(calls_of(sources(fmt, LW, LH)[:1], F)[0])
        assert L.dsv1_resladder_set_levels(r.h, C.byref(other)) == DSVG_ERR_ARG and L.dsv1_resladder_set_levels(r.h, None) == DSVG_ERR_ARG
        r.collect()
        r.set_levels(None)
    finally:
        r.close()
    # the standalone calls
    src = LV.noise(1, 8, 6, fmt, 2)
    dst = np.zeros_like(src)
    hist = np.zeros((1, 3, 256), dtype=np.uint32)
    assert L.dsv1_levels_clip(0, None, 8, 6, fmt, 1, dst.ctypes.data, C.byref(grade), 0) == DSVG_ERR_ARG
    assert L.dsv1_levels_clip(0, src.ctypes.data, 8, 6, fmt, 1, None, C.byref(grade), 0) == DSVG_ERR_ARG
    assert L.dsv1_levels_clip(0, src.ctypes.data, 8, 6, fmt, 1, dst.ctypes.data, None, 0) == DSVG_ERR_ARG
    assert L.dsv1_levels_clip(0, None, 8, 6, fmt, 1, None, C.byref(grade), 1) == DSVG_ERR_ARG
    for n in (0, -1):
        assert L.dsv1_levels_clip(0, src.ctypes.data, 8, 6, fmt, n, dst.ctypes.data, C.byref(grade), 0) == DSVG_ERR_ARG
        assert L.dsv1_histogram_clip(0, src.ctypes.data, 8, 6, fmt, n, hist.ctypes.data, 0) == DSVG_ERR_ARG
    assert L.dsv1_levels_clip(0, src.ctypes.data, 8, 6, 0x7, 1, dst.ctypes.data, C.byref(grade), 0) == DSVG_ERR_ARG
    assert L.dsv1_histogram_clip(0, src.ctypes.data, 0, 6, fmt, 1, hist.ctypes.data, 0) == DSVG_ERR_ARG
    assert L.dsv1_histogram_clip(0, src.ctypes.data, 8, 6, fmt, 1, None, 0) == DSVG_ERR_ARG
    assert not dst.any() and not hist.any()


def test_feature_off(pkg, orc):
    """a batch that never calls the setter, and one that set and cleared levels, write the oracle's streams of the clip itself; neither
    holds a lane"""
    fmt = A.SUBSAMP_420
    L = pkg.lib()
    clips = sources(fmt, W, H)
    want = [oracle(("off", s), clips[s], W, H, fmt, qp=80)[0] for s in range(S)]
    calls = calls_of(clips, F)
    cfg = pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80))
    for mode in ("never", "cleared", "cleared by the identity"):
        b = pkg.Batch(cfg, S, F)
        try:
            if mode != "never":
                b.set_source_levels(lv_of(pkg, T_GRADE))
                assert L.dsv1_batch_has_source_lane(b.h)
                b.set_source_levels(None if mode == "cleared" else pkg.Levels.identity())
            assert not L.dsv1_batch_has_source_lane(b.h), mode
            pin = b.pinned(calls[0].shape)
            pin[...] = calls[0]
            assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == 0, mode                                            # nothing set: stage works
            b.submit(pin)
            first = b.collect()
            got = [bytes(x) + bytes(y) for x, y in zip(first, b.encode(calls[1]))]
        finally:
            b.close()
        assert got == want, mode
