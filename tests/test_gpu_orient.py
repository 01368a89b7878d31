"""The orientation pass on the GPU (include/dsv1_api.h, Orientation; csrc/k_orient.hip): dsv1_orient_clip equals the numpy statement
tests/_orient.py, touching nothing around its buffers; batches, quality ladders, chain mode and resolution ladders with an orientation
set write the packets of the same session fed the numpy-oriented clip, which are the oracle's streams of it."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import _chroma as CH
import _deint as DI
import _denoise as D
import _orient as O
import _pixfmt as PF
import _reframe as R
import _rgb as RG
import _scale as Z

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2
CRF = dict(gop=4, rc_mode_cli=1, scd=1)
S, F = 2, 4
RW, RH, MW, MH = 50, 70, 70, 50                           # the sessions' raw (portrait) and oriented geometry
CW, CH_ = 96, 64                                          # the canvas of the sessions with a reframe behind
GUARD = 64


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


def cs(pkg, r):
    return pkg.Reframe(r["in_w"], r["in_h"], (r["x"], r["y"], r["w"], r["h"]), (r["out_w"], r["out_h"]), (r["dst_x"], r["dst_y"]), r["fill"])


# ---- the standalone call ---------------------------------------------------------------------------------------------------------
def check_clip(pkg, mem, orient, fmt, w, h, n):
    fb = A.frame_bytes(w, h, fmt)
    src = O.noise(n, w, h, fmt, 0x0A0 + 8 * fmt + orient)
    want = O.orient_clip(src, w, h, fmt, orient)
    tag = "%s 0x%x %dx%d" % (O.NAMES[orient], fmt, w, h)
    # host memory: the output between 64 sentinel bytes on each side
    big = np.full(2 * GUARD + want.size, 0xC3, dtype=np.uint8)
    out = big[GUARD:GUARD + want.size]
    pkg.orient_clip(src, w, h, fmt, orient, out=out)
    assert (big[:GUARD] == 0xC3).all() and (big[GUARD + want.size:] == 0xC3).all(), "written outside the destination (host) " + tag
    A.assert_same("host " + tag, out.reshape(want.shape), want)
    # device memory: source and destination exactly as long as their contents, at two alignments each; the source ends where its
    # allocation's pattern begins, so a load past the last frame would show (in the result, were it used)
    for soff, doff in ((256, GUARD), (256 + 3, GUARD + 5)):
        big_s = np.full(soff + n * fb + 64, 0x99, dtype=np.uint8)
        big_s[soff:soff + n * fb] = src.reshape(-1)
        big_d = np.full(doff + want.size + GUARD, 0x3C, dtype=np.uint8)
        ps, pd = mem.alloc(big_s), mem.alloc(big_d)
        pkg.orient_clip(C.c_void_p(ps.value + soff), w, h, fmt, orient, n=n, out=C.c_void_p(pd.value + doff))
        after = mem.read(pd, big_d.size)
        assert (after[:doff] == 0x3C).all() and (after[doff + want.size:] == 0x3C).all(), "written outside the destination (device) " + tag
        A.assert_same("device offsets %d %d %s" % (soff, doff, tag), after[doff:doff + want.size].reshape(want.shape), want)
        assert np.array_equal(mem.read(ps, big_s.size), big_s)


CODES = [(o, f) for o in range(1, 8) for f in O.FORMATS if O.valid(o, f)]


@pytest.mark.parametrize("orient,fmt", CODES, ids=["%s-0x%x" % (O.NAMES[o], f) for o, f in CODES])
def test_orient_clip_equals_numpy(pkg, mem, orient, fmt):
    for w, h in O.GEOMS:
        check_clip(pkg, mem, orient, fmt, w, h, 3)


@pytest.mark.parametrize("orient", [O.ROT90, O.HFLIP], ids=["rot90", "hflip"])
def test_orient_clip_equals_numpy_1080p(pkg, mem, orient):
    check_clip(pkg, mem, orient, A.SUBSAMP_420, 1920, 1080, 2)


def test_code_0_copies(pkg, mem):
    for fmt in O.FORMATS:
        check_clip(pkg, mem, O.NONE, fmt, 70, 50, 3)


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
    """the packets of the same session fed the numpy-oriented clips, nothing set"""
    b = make()
    try:
        return run(b, calls_of(clips, F), form, pipelined)
    finally:
        b.close()


def test_plain_batch(pkg, orc):
    fmt = A.SUBSAMP_420
    clips = sources(fmt, RW, RH)
    turned = [O.orient_clip(c, RW, RH, fmt, O.ROT90) for c in clips]
    want = [oracle(("b", s), turned[s], MW, MH, fmt, qp=80)[0] for s in range(S)]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(MW, MH, fmt, **dict(CRF, qp=80)), S, F)
    assert fed(make, turned) == want
    calls = calls_of(clips, F)
    assert len(calls) == 2
    for form, pipelined in (("host", True), ("host", False), ("device", False), ("held", True)):
        b = make()
        try:
            b.set_source_orient(pkg.Orient.ROT90)
            assert b.in_dims == (RW, RH) and b.frame_bytes == A.frame_bytes(RW, RH, fmt)
            got = run(b, calls, form, pipelined)
        finally:
            b.close()
        assert got == want, (form, pipelined)


@pytest.mark.parametrize("orient", [O.ROT270, O.HFLIP], ids=["rot270", "hflip"])
def test_quality_ladder_and_chain_mode(pkg, orc, orient):
    fmt = A.SUBSAMP_420
    qps = (60, 90)
    rw, rh = O.dims(O.inverse(orient), MW, MH)
    clips = sources(fmt, rw, rh)
    turned = [O.orient_clip(c, rw, rh, fmt, orient) for c in clips]
    calls = calls_of(clips, F)
    rungs = [pkg.make_encoder_cfg(MW, MH, fmt, **dict(CRF, qp=q)) for q in qps]
    want = [oracle(("l", orient, s, q), turned[s], MW, MH, fmt, qp=q)[0] for s in range(S) for q in qps]
    assert fed(lambda: pkg.Ladder(rungs, S, F), turned) == want
    for form in ("host", "held"):
        b = pkg.Ladder(rungs, S, F)
        try:
            b.set_source_orient(orient)
            assert b.in_dims == (rw, rh)
            got = run(b, calls, form)
        finally:
            b.close()
        assert got == want, form
    want = oracle(("c", orient), turned[0], MW, MH, fmt, qp=75)[0]
    cfg = pkg.make_encoder_cfg(MW, MH, fmt, **dict(CRF, qp=75))
    for form in ("host", "device"):
        b = pkg.Batch(cfg, 1, F, chains=2)
        try:
            b.set_source_orient(orient)
            got = run(b, [c[:1] for c in calls], form, pipelined=False)
        finally:
            b.close()
        assert got[0] == want, form


def cpf(pkg, f):
    return pkg.PixFormat(f["layout"], f["depth"], f["msb"], f["pitch"], f["frame_bytes"])


def test_behind_a_uyvy_422_source_halved_to_420(pkg, orc):
    """the documented route of a 4:2:2 source to a rotation: the converter halves its chroma in front of the pass; the format is set
    AFTER the orientation and resolves at the raw geometry"""
    fmt, sfmt = A.SUBSAMP_420, A.SUBSAMP_422
    f = PF.pf(PF.UYVY)
    planar = sources(sfmt, RW, RH)
    raws = [PF.pack(c.astype(np.uint32), f, RW, RH, sfmt, np.random.default_rng(s)).reshape(c.shape[0], -1) for s, c in enumerate(planar)]
    conv = [CH.convert_sub(r.reshape(-1), f, RW, RH, sfmt, fmt, r.shape[0]) for r in raws]
    turned = [O.orient_clip(c, RW, RH, fmt, O.ROT90) for c in conv]
    want = [oracle(("u", s), turned[s], MW, MH, fmt, qp=80)[0] for s in range(S)]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(MW, MH, fmt, **dict(CRF, qp=80)), S, F)
    assert fed(make, turned) == want
    for form in ("host", "device"):
        b = make()
        try:
            b.set_source_orient(O.ROT90)
            b.set_source_format(cpf(pkg, f), src_subsamp=sfmt)
            assert b.frame_bytes == raws[0].shape[1]
            got = run(b, calls_of(raws, F), form)
        finally:
            b.close()
        assert got == want, form


def test_behind_an_rgb_source(pkg, orc):
    fmt, n = A.SUBSAMP_420, 2 * F
    f = RG.rf(RG.BGRA, RG.BT709, 0)
    raws, turned = [], []
    for s in range(S):
        rgb = A.gen_clip(RW, RH, A.SUBSAMP_444, 0x5C0 + s, n, style=1)
        Rr, G, B = (rgb[:, k * RW * RH:(k + 1) * RW * RH].reshape(n, RH, RW) for k in range(3))
        raw = RG.pack(Rr, G, B, f, RW, RH, np.random.default_rng(s))
        raws.append(raw.reshape(n, -1))
        turned.append(O.orient_clip(RG.import_(raw, f, RW, RH, fmt, n), RW, RH, fmt, O.TRANSVERSE))
    want = [oracle(("rgb", s), turned[s], MW, MH, fmt, qp=80)[0] for s in range(S)]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(MW, MH, fmt, **dict(CRF, qp=80)), S, F)
    assert fed(make, turned) == want
    for form in ("host", "held"):
        b = make()
        try:
            b.set_source_orient(O.TRANSVERSE)
            b.set_source_rgb(pkg.RgbFormat(f["order"], f["matrix"], f["full"], f["upsample"], f["pitch"], f["frame_bytes"]))
            got = run(b, calls_of(raws, F), form)
        finally:
            b.close()
        assert got == want, form


def test_behind_the_deinterlacer_and_the_noise_filter_across_two_calls(pkg, orc):
    """field-rate deinterlacer -> noise filter -> ROT180, two calls: the deinterlacer's history and the filter's state cross the call
    boundary at the RAW geometry, in front of the orientation"""
    fmt, dn = A.SUBSAMP_420, (24, 24)
    clips = [DI.gen_interlaced(MW, MH, fmt, F, 0x1F0 + s, 1) for s in range(S)]            # F input frames = 2 F pictures
    den = [D.denoise_clip(DI.deint_clip(c, MW, MH, fmt, DI.FIELD, 1), MW, MH, fmt, *dn)[0] for c in clips]
    cut = D.denoise_clip(DI.deint_clip(clips[0][F // 2:], MW, MH, fmt, DI.FIELD, 1), MW, MH, fmt, *dn)[0]
    assert not np.array_equal(den[0][F:], cut)           # (the second call's history and state matter)
    turned = [O.orient_clip(c, MW, MH, fmt, O.ROT180) for c in den]
    want = [oracle(("all", s), turned[s], MW, MH, fmt, qp=80)[0] for s in range(S)]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(MW, MH, fmt, **dict(CRF, qp=80)), S, F)
    assert fed(make, turned) == want
    calls = calls_of(clips, F // 2)
    assert len(calls) == 2
    for form in ("host", "device"):
        b = make()
        try:
            b.set_source_orient(O.ROT180)
            b.set_source_deinterlace(pkg.Deint(DI.FIELD, 1))
            b.set_source_denoise(pkg.Denoise(*dn))
            got = run(b, calls, form, pipelined=form == "host")
        finally:
            b.close()
        assert got == want, form


RF = R.rf(MW, MH, (6, 4, 51, 33), (CW, CH_), (10, 8))     # the reframe test's window of the 70 x 50 picture on its 96 x 64 canvas


def test_with_the_reframe_behind_it(pkg, orc):
    fmt = A.SUBSAMP_420
    clips = sources(fmt, RW, RH)
    framed = [R.reframe_clip(O.orient_clip(c, RW, RH, fmt, O.ROT90), RF, fmt) for c in clips]
    want = [oracle(("rf", s), framed[s], CW, CH_, fmt, qp=80)[0] for s in range(S)]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(CW, CH_, fmt, **dict(CRF, qp=80)), S, F)
    assert fed(make, framed) == want
    for form in ("host", "device", "held"):
        b = make()
        try:
            b.set_source_reframe(cs(pkg, RF))            # FIRST: its input is the oriented geometry
            b.set_source_orient(O.ROT90)
            assert b.in_dims == (RW, RH) and b.frame_bytes == A.frame_bytes(RW, RH, fmt)
            got = run(b, calls_of(clips, F), form, pipelined=form != "device")
        finally:
            b.close()
        assert got == want, form


# ---- resolution ladder: a 96 x 128 portrait source stood upright (128 x 96); with a reframe, pillarboxed onto 192 x 96 ----
LRW, LRH, LW, LH, LCW, LCH = 96, 128, 128, 96, 192, 96
LRF = R.rf(LW, LH, (0, 0, LW, LH), (LCW, LCH), (32, 0))


def ladder_run(b, calls, form):
    dev = form != "host"
    ins = [b.upload(c) for c in calls] if dev else calls
    got, xs, xm = [b""] * b.nstreams, [], []
    for c in ins:
        b.submit(c, on_device=dev, held=form == "held")
    for _ in ins:
        got[:] = [x + bytes(p) for x, p in zip(got, b.collect())]
        xs.append(b.src_sse())
        xm.append(b.src_ssim_fx())
    return got, np.concatenate(xs, axis=1), np.concatenate(xm, axis=1)


@pytest.mark.parametrize("framed", [False, True], ids=["oriented", "oriented-reframed"])
def test_resolution_ladder(pkg, orc, framed):
    fmt = A.SUBSAMP_420
    sw, sh = (LCW, LCH) if framed else (LW, LH)          # what stands for the source behind the chain
    shapes = [(sw, sh, 80), (sw // 2, sh // 2, 70)]      # one geometry of the (oriented) source's own size
    clips = sources(fmt, LRW, LRH)
    turned = [O.orient_clip(c, LRW, LRH, fmt, O.ROT90) for c in clips]
    if framed:
        turned = [R.reframe_clip(c, LRF, fmt) for c in turned]
    want = []
    for s, clip in enumerate(turned):
        for gw, gh, qp in shapes:
            sc = clip if (gw, gh) == (sw, sh) else Z.scale_clip(clip, sw, sh, fmt, gw, gh, Z.CUBIC)
            want.append(oracle(("r", framed, s, gw), sc, gw, gh, fmt, qp=qp)[0])
    geoms = lambda: [(gw, gh, [pkg.make_encoder_cfg(gw, gh, fmt, **dict(CRF, qp=qp))]) for gw, gh, qp in shapes]
    # the ladder fed the oriented clip: packets and source-resolution figures to compare with
    b = pkg.ResLadder(sw, sh, fmt, geoms(), S, F, Z.CUBIC)
    try:
        b.src_quality_enable(sse=True, ssim=True, filt=Z.CUBIC)
        base, bsse, bssim = ladder_run(b, calls_of(turned, F), "host")
    finally:
        b.close()
    assert base == want
    for form in ("host", "held"):
        b = pkg.ResLadder(LRW, LRH, fmt, geoms(), S, F, Z.CUBIC, orient=O.ROT90, reframe=cs(pkg, LRF) if framed else None)
        try:
            assert (b.width, b.height) == (sw, sh) and b.frame_bytes == A.frame_bytes(LRW, LRH, fmt)
            b.src_quality_enable(sse=True, ssim=True, filt=Z.CUBIC)
            got, xsse, xssim = ladder_run(b, calls_of(clips, F), form)
            up = b.uploads()
        finally:
            b.close()
        assert got == want, form
        assert np.array_equal(xsse, bsse) and np.array_equal(xssim, bssim), form
        assert up == ((2 * S * F * A.frame_bytes(LRW, LRH, fmt), 2) if form == "host" else (0, 0))


# ---- errors and the feature off --------------------------------------------------------------------------------------------------
def test_error_contract(pkg, orc):
    fmt = A.SUBSAMP_420
    L = pkg.lib()
    clips = sources(fmt, RW, RH)
    turned = O.orient_clip(clips[0], RW, RH, fmt, O.ROT90)
    want = oracle(("b", 0), turned, MW, MH, fmt, qp=80)[0]
    own = sources(fmt, MW, MH)[:1]
    plain = oracle(("p", 0), own[0], MW, MH, fmt, qp=80)[0]
    cfg = pkg.make_encoder_cfg(MW, MH, fmt, **dict(CRF, qp=80))
    calls = calls_of(clips[:1], F)
    setter = L.dsv1_batch_set_source_orient
    b = pkg.Batch(cfg, 1, F)
    try:
        # a code that is none: refused, and the next submit behaves as before (nothing set)
        for bad in (-1, 8, 64):
            assert setter(b.h, bad) == DSVG_ERR_ARG
        assert not L.dsv1_batch_has_source_lane(b.h)
        p1 = bytes(b.encode(calls_of(own, F)[0])[0])
        assert p1 and plain.startswith(p1)
        # a pass already set
        b.set_source_denoise(pkg.Denoise(24, 24))
        assert setter(b.h, O.ROT90) == DSVG_ERR_ARG
        b.set_source_denoise(None)
        b.set_source_deinterlace(pkg.Deint(DI.FRAME, 1))
        assert setter(b.h, O.ROT90) == DSVG_ERR_ARG
        b.set_source_deinterlace(None)
        b.set_source_ivtc(pkg.Ivtc(1, 0))
        assert setter(b.h, O.ROT90) == DSVG_ERR_ARG
        b.set_source_ivtc(None)
        b.set_source_format(pkg.PixFormat(PF.UYVY), src_subsamp=A.SUBSAMP_422)
        assert setter(b.h, O.ROT90) == DSVG_ERR_ARG
        b.set_source_format(None)
        # a clip staged
        pin = b.pinned((1, F, A.frame_bytes(MW, MH, fmt)))
        pin[...] = calls_of(own, F)[1]
        assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == 0
        assert setter(b.h, O.ROT90) == DSVG_ERR_ARG
        b.submit(pin)
        assert setter(b.h, O.ROT90) == DSVG_ERR_ARG                                                             # a batch in flight
        assert p1 + bytes(b.collect()[0]) == plain       # every refusal left the batch as it was: it codes the clips themselves
        assert not L.dsv1_batch_has_source_lane(b.h)
    finally:
        b.close()
    b = pkg.Batch(cfg, 1, F)
    try:
        b.set_source_orient(O.ROT90)
        assert L.dsv1_batch_has_source_lane(b.h)
        pin = b.pinned(calls[0].shape)
        pin[...] = calls[0]
        assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == DSVG_ERR_ARG                                          # stage is refused while set
        onto = cs(pkg, R.rf(80, 60, (4, 4, MW, MH), (MW, MH)))
        assert L.dsv1_reframe_valid(C.byref(onto), fmt)
        assert L.dsv1_batch_set_source_reframe(b.h, C.byref(onto)) == DSVG_ERR_ARG                               # a reframe comes BEFORE it
        assert L.dsv1_batch_set_source_reframe(b.h, None) == DSVG_ERR_ARG
        b.submit(pin)
        for x in (O.NONE, O.HFLIP, O.ROT90, -1, 8):                                                              # in flight, invalid: as it was
            assert setter(b.h, x) == DSVG_ERR_ARG
        first = b.collect()[0]
        for bad in (-1, 8):
            assert setter(b.h, bad) == DSVG_ERR_ARG
        b.set_source_denoise(pkg.Denoise(24, 24))                                                                 # set after it: fine; then it is locked
        assert setter(b.h, O.NONE) == DSVG_ERR_ARG
        b.set_source_denoise(None)
        assert bytes(first) + bytes(b.encode(calls[1])[0]) == want
    finally:
        b.close()
    # a transposing code on a 4:2:2 and on a 4:1:1 batch; a mirror is fine there
    for sub in (A.SUBSAMP_422, A.SUBSAMP_411):
        w, h = 64, 48
        clip = A.gen_clip(w, h, sub, 0x610 + sub, F, style=1)
        b = pkg.Batch(pkg.make_encoder_cfg(w, h, sub, **dict(CRF, qp=80)), 1, F)
        try:
            for code in (O.TRANSPOSE, O.ROT90, O.ROT270, O.TRANSVERSE):
                assert setter(b.h, code) == DSVG_ERR_ARG
            assert not L.dsv1_batch_has_source_lane(b.h)
            assert bytes(b.encode(clip[None])[0]) == oracle(("sub", sub), clip, w, h, sub, qp=80)[0]
        finally:
            b.close()
        b = pkg.Batch(pkg.make_encoder_cfg(w, h, sub, **dict(CRF, qp=80)), 1, F)
        try:
            b.set_source_orient(O.VFLIP)
            assert setter(b.h, O.ROT90) == DSVG_ERR_ARG                                                          # ... and VFLIP stays
            flipped = O.orient_clip(clip, w, h, sub, O.VFLIP)
            assert bytes(b.encode(clip[None])[0]) == oracle(("subflip", sub), flipped, w, h, sub, qp=80)[0]
        finally:
            b.close()
    # the resolution ladder's open
    meta = pkg.Meta()
    meta.width, meta.height, meta.subsamp = LRW, LRH, fmt
    h = C.c_void_p(None)

    def open_(m, orient, rfr, gw, gh, pf=None, rgb=None):
        enc = (pkg.Encoder * 1)(pkg.make_encoder_cfg(gw, gh, fmt, **dict(CRF, qp=80)))
        rr = (pkg.ResRung * 1)(pkg.ResRung(gw, gh, 1, enc))
        return L.dsv1_resladder_open_oriented(C.byref(h), C.byref(m), orient, C.byref(rfr) if rfr is not None else None, pf, fmt, rgb, rr, 1, 0, 1,
                                              F, Z.CUBIC)

    raw_in = cs(pkg, R.rf(LRW, LRH, (0, 0, LRW, LRH), (LCW, 128), (48, 0)))                                      # its input is the RAW geometry
    assert open_(meta, O.ROT90, raw_in, LCW, 128) == DSVG_ERR_ARG and h.value is None
    assert open_(meta, O.NONE, cs(pkg, LRF), LCW, LCH) == DSVG_ERR_ARG and h.value is None                       # oriented by 0: 96 x 128 again
    assert open_(meta, 8, None, LW, LH) == DSVG_ERR_ARG and h.value is None
    assert open_(meta, O.ROT90, None, LRW, LRH) == DSVG_ERR_ARG and h.value is None                              # 96 x 128 is no downscale of 128 x 96
    m422 = pkg.Meta()
    m422.width, m422.height, m422.subsamp = LRW, LRH, A.SUBSAMP_422
    assert open_(m422, O.ROT90, None, LW, LH) == DSVG_ERR_ARG and h.value is None
    assert open_(meta, O.ROT90, cs(pkg, LRF), LCW, LCH) == 0 and h.value is not None
    L.dsv1_resladder_close(h)
    # the standalone call
    src = O.noise(1, 8, 6, fmt, 2)
    dst = np.zeros_like(src)
    assert L.dsv1_orient_clip(0, None, 8, 6, fmt, 1, dst.ctypes.data, O.ROT90, 0) == DSVG_ERR_ARG
    assert L.dsv1_orient_clip(0, src.ctypes.data, 8, 6, fmt, 1, None, O.ROT90, 0) == DSVG_ERR_ARG
    assert L.dsv1_orient_clip(0, None, 8, 6, fmt, 1, None, O.ROT90, 1) == DSVG_ERR_ARG
    for n in (0, -1):
        assert L.dsv1_orient_clip(0, src.ctypes.data, 8, 6, fmt, n, dst.ctypes.data, O.ROT90, 0) == DSVG_ERR_ARG
    assert L.dsv1_orient_clip(0, src.ctypes.data, 8, 6, A.SUBSAMP_422, 1, dst.ctypes.data, O.ROT90, 0) == DSVG_ERR_ARG
    assert not dst.any()


def test_feature_off(pkg, orc):
    """a batch that never calls the setter, one that sets code 0, and one that set and cleared a code write the oracle's streams of the
    clip itself; none of them holds a lane"""
    fmt = A.SUBSAMP_420
    L = pkg.lib()
    clips = sources(fmt, MW, MH)
    want = [oracle(("off", s), clips[s], MW, MH, fmt, qp=80)[0] for s in range(S)]
    calls = calls_of(clips, F)
    cfg = pkg.make_encoder_cfg(MW, MH, fmt, **dict(CRF, qp=80))
    for mode in ("never", "code 0", "cleared"):
        b = pkg.Batch(cfg, S, F)
        try:
            if mode == "code 0":
                b.set_source_orient(O.NONE)
            if mode == "cleared":
                b.set_source_orient(O.ROT90)
                assert L.dsv1_batch_has_source_lane(b.h) and b.in_dims == (RW, RH)
                b.set_source_orient(O.NONE)
            assert not L.dsv1_batch_has_source_lane(b.h), mode
            assert b.in_dims == (MW, MH) and b.frame_bytes == A.frame_bytes(MW, MH, fmt)
            pin = b.pinned(calls[0].shape)
            pin[...] = calls[0]
            assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == 0, mode                                            # nothing set: stage works
            b.submit(pin)
            first = b.collect()
            got = [bytes(x) + bytes(y) for x, y in zip(first, b.encode(calls[1]))]
        finally:
            b.close()
        assert got == want, mode
