"""Reframe and line sums on the GPU (include/dsv1_api.h, Reframe; csrc/k_reframe.hip): dsv1_reframe_clip and dsv1_line_sums_clip equal
the numpy statement tests/_reframe.py, touching nothing around their buffers; batches, quality ladders, chain mode and resolution
ladders with a reframe set write the packets of the same session fed the numpy-reframed clip, which are the oracle's streams of it."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import _deint as DI
import _denoise as D
import _pixfmt as PF
import _reframe as R
import _resample as RS
import _rgb as RG
import _scale as Z

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2
CRF = dict(gop=4, rc_mode_cli=1, scd=1)
S, F = 2, 4
IW, IH, OW, OH = 70, 50, 96, 64                           # the sessions' input and canvas
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


# ---- the standalone calls ------------------------------------------------------------------------------------------------------
CASES = [(name, r, n, fmt) for name, r, n in R.gpu_cases() for fmt in (R.formats_of(r) if r["in_w"] < 1920 else [A.SUBSAMP_420])]


@pytest.mark.parametrize("name,r,n,fmt", CASES, ids=["%s-0x%x" % (c[0], c[3]) for c in CASES])
def test_reframe_clip_equals_numpy(pkg, mem, name, r, n, fmt):
    ifb = A.frame_bytes(r["in_w"], r["in_h"], fmt)
    src = R.noise(n, r["in_w"], r["in_h"], fmt, 0x2F0 + fmt)
    want = R.reframe_clip(src, r, fmt)
    # host memory: the output between 64 sentinel bytes on each side
    big = np.full(2 * GUARD + want.size, 0xC3, dtype=np.uint8)
    out = big[GUARD:GUARD + want.size]
    pkg.reframe_clip(src, cs(pkg, r), fmt, out=out)
    assert (big[:GUARD] == 0xC3).all() and (big[GUARD + want.size:] == 0xC3).all(), "written outside the destination (host)"
    A.assert_same("host", out.reshape(want.shape), want)
    # device memory: source and destination exactly as long as their contents, at two alignments each; the source ends where its
    # allocation's pattern begins, so a load past the last frame would show (in the result, were it used)
    for soff, doff in ((256, GUARD), (256 + 3, GUARD + 5)):
        big_s = np.full(soff + n * ifb + 64, 0x99, dtype=np.uint8)
        big_s[soff:soff + n * ifb] = src.reshape(-1)
        big_d = np.full(doff + want.size + GUARD, 0x3C, dtype=np.uint8)
        ps, pd = mem.alloc(big_s), mem.alloc(big_d)
        pkg.reframe_clip(C.c_void_p(ps.value + soff), cs(pkg, r), fmt, n=n, out=C.c_void_p(pd.value + doff))
        after = mem.read(pd, big_d.size)
        assert (after[:doff] == 0x3C).all() and (after[doff + want.size:] == 0x3C).all(), "written outside the destination (device)"
        A.assert_same("device offsets %d %d" % (soff, doff), after[doff:doff + want.size].reshape(want.shape), want)
        assert np.array_equal(mem.read(ps, big_s.size), big_s)


_sums = {}


def sum_case(w, h):
    """3 frames that differ, and their numpy sums: computed once, shared"""
    if (w, h) not in _sums:
        clip = R.noise(3, w, h, A.SUBSAMP_420, 0x11 + w)
        clip[1, :w * h] //= 2                             # (frames of another level each: mixed-up frames would show)
        clip[2, :w * h] |= 0x80
        _sums[(w, h)] = clip, R.line_sums(clip, w, h, A.SUBSAMP_420)
    return _sums[(w, h)]


@pytest.mark.parametrize("w,h", R.LINE_SUM_GEOMS)
def test_line_sums_clip_equals_numpy(pkg, mem, w, h):
    fmt = A.SUBSAMP_420
    clip, (rows, cols) = sum_case(w, h)
    assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[1], rows[2])
    for n in (1, 3):
        gr, gc = pkg.line_sums_clip(clip[:n], w, h, fmt)
        assert gr.dtype == np.uint32 and gr.shape == (n, h) and gc.shape == (n, w)
        assert np.array_equal(gr, rows[:n]) and np.array_equal(gc, cols[:n]), "host, n = %d" % n
    # device memory at an odd address, the clip ending with its allocation's contents
    big = np.full(259 + clip.size, 0x77, dtype=np.uint8)
    big[259:] = clip.reshape(-1)
    p = mem.alloc(big)
    gr, gc = pkg.line_sums_clip(C.c_void_p(p.value + 259), w, h, fmt, n=3)
    assert np.array_equal(gr, rows) and np.array_equal(gc, cols), "device"


def test_line_sums_do_not_overflow_or_saturate(pkg):
    w, h, fmt = 48, 520, A.SUBSAMP_444
    clip = np.full((2, A.frame_bytes(w, h, fmt)), 255, dtype=np.uint8)
    rows, cols = pkg.line_sums_clip(clip, w, h, fmt)
    assert (rows == 255 * w).all() and (cols == 255 * h).all() and 255 * h > 65535


@pytest.mark.parametrize("rect", [(0, 36, 352, 216), (48, 0, 256, 288)], ids=["letterbox", "pillarbox"])
def test_detect_bars_clip(pkg, mem, rect):
    w, h, fmt = 352, 288, A.SUBSAMP_420
    clip = R.boxed(3, w, h, fmt, rect, 0xBA5)
    rows, cols = R.line_sums(clip, w, h, fmt)
    for thresh, align in ((24, 2), (24, 16), (60, 64)):
        want = R.bars_from_sums(rows, cols, thresh, align)
        assert pkg.detect_bars_clip(clip, w, h, fmt, thresh, align) == want
        assert pkg.bars_from_sums(*pkg.line_sums_clip(clip, w, h, fmt), thresh, align) == want
    assert R.bars_from_sums(rows, cols, 24, 2) == rect
    p = mem.alloc(clip)
    assert pkg.detect_bars_clip(p, w, h, fmt, 24, 2, n=3) == rect
    black = np.full_like(clip, 16)
    assert pkg.detect_bars_clip(black, w, h, fmt, 24, 2) is None


# ---- sessions ------------------------------------------------------------------------------------------------------------------
_cache = {}
RF = R.rf(IW, IH, (6, 4, 51, 33), (OW, OH), (10, 8))


def sources(fmt, w=IW, h=IH, n=2 * F):
    key = ("src", fmt, w, h, n)
    if key not in _cache:
        _cache[key] = [A.gen_clip(w, h, fmt, 0x2E0 + s, n, style=s & 1) for s in range(S)]
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


def fed_framed(pkg, make, framed, form="host", pipelined=True):
    """the packets of the same session fed the numpy-reframed clips, nothing set"""
    b = make()
    try:
        return run(b, calls_of(framed, F), form, pipelined)
    finally:
        b.close()


def test_plain_batch(pkg, orc):
    fmt = A.SUBSAMP_420
    clips = sources(fmt)
    framed = [R.reframe_clip(c, RF, fmt) for c in clips]
    want = [oracle(("b", s), framed[s], OW, OH, fmt, qp=80)[0] for s in range(S)]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(OW, OH, fmt, **dict(CRF, qp=80)), S, F)
    assert fed_framed(pkg, make, framed) == want
    calls = calls_of(clips, F)
    assert len(calls) == 2
    for form in ("host", "device", "held"):
        b = make()
        try:
            b.set_source_reframe(cs(pkg, RF))
            assert b.in_dims == (IW, IH) and b.frame_bytes == A.frame_bytes(IW, IH, fmt)
            got = run(b, calls, form, pipelined=form != "device")
        finally:
            b.close()
        assert got == want, form


def test_quality_ladder_and_chain_mode(pkg, orc):
    fmt = A.SUBSAMP_420
    qps = (60, 90)
    clips = sources(fmt)
    framed = [R.reframe_clip(c, RF, fmt) for c in clips]
    calls = calls_of(clips, F)
    rungs = [pkg.make_encoder_cfg(OW, OH, fmt, **dict(CRF, qp=q)) for q in qps]
    want = [oracle(("l", s, q), framed[s], OW, OH, fmt, qp=q)[0] for s in range(S) for q in qps]
    assert fed_framed(pkg, lambda: pkg.Ladder(rungs, S, F), framed) == want
    for form in ("host", "held"):
        b = pkg.Ladder(rungs, S, F)
        try:
            b.set_source_reframe(cs(pkg, RF))
            got = run(b, calls, form)
        finally:
            b.close()
        assert got == want, form
    want = oracle(("c",), framed[0], OW, OH, fmt, qp=75)[0]
    cfg = pkg.make_encoder_cfg(OW, OH, fmt, **dict(CRF, qp=75))
    for form in ("host", "device"):
        b = pkg.Batch(cfg, 1, F, chains=2)
        try:
            b.set_source_reframe(cs(pkg, RF))
            got = run(b, [c[:1] for c in calls], form, pipelined=False)
        finally:
            b.close()
        assert got[0] == want, form


def _uyvy(clips, w, h, fmt):
    f = PF.pf(PF.UYVY)
    raws = [PF.pack(c.astype(np.uint32), f, w, h, fmt, np.random.default_rng(s)).reshape(c.shape[0], -1) for s, c in enumerate(clips)]
    for r, c in zip(raws, clips):
        assert np.array_equal(PF.convert(r.reshape(-1), f, w, h, fmt, c.shape[0]), c)
    return raws, f


def test_behind_a_uyvy_source(pkg, orc):
    """the format is set AFTER the reframe and resolves at the input geometry"""
    fmt = A.SUBSAMP_422
    clips = sources(fmt)
    raws, f = _uyvy(clips, IW, IH, fmt)
    framed = [R.reframe_clip(c, RF, fmt) for c in clips]
    want = [oracle(("u", s), framed[s], OW, OH, fmt, qp=80)[0] for s in range(S)]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(OW, OH, fmt, **dict(CRF, qp=80)), S, F)
    assert fed_framed(pkg, make, framed) == want
    for form in ("host", "device"):
        b = make()
        try:
            b.set_source_reframe(cs(pkg, RF))
            b.set_source_format(pkg.PixFormat(f["layout"], f["depth"], f["msb"], f["pitch"], f["frame_bytes"]))
            assert b.frame_bytes == raws[0].shape[1]
            got = run(b, calls_of(raws, F), form)
        finally:
            b.close()
        assert got == want, form


def test_behind_an_rgb_source(pkg, orc):
    fmt, n = A.SUBSAMP_420, 2 * F
    f = RG.rf(RG.BGRA, RG.BT709, 0)
    raws, framed = [], []
    for s in range(S):
        rgb = A.gen_clip(IW, IH, A.SUBSAMP_444, 0x3C0 + s, n, style=1)
        Rr, G, B = (rgb[:, k * IW * IH:(k + 1) * IW * IH].reshape(n, IH, IW) for k in range(3))
        raw = RG.pack(Rr, G, B, f, IW, IH, np.random.default_rng(s))
        raws.append(raw.reshape(n, -1))
        framed.append(R.reframe_clip(RG.import_(raw, f, IW, IH, fmt, n), RF, fmt))
    want = [oracle(("rgb", s), framed[s], OW, OH, fmt, qp=80)[0] for s in range(S)]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(OW, OH, fmt, **dict(CRF, qp=80)), S, F)
    assert fed_framed(pkg, make, framed) == want
    for form in ("host", "held"):
        b = make()
        try:
            b.set_source_reframe(cs(pkg, RF))
            b.set_source_rgb(pkg.RgbFormat(f["order"], f["matrix"], f["full"], f["upsample"], f["pitch"], f["frame_bytes"]))
            got = run(b, calls_of(raws, F), form)
        finally:
            b.close()
        assert got == want, form


def test_all_passes_across_two_calls(pkg, orc):
    """UYVY -> field-rate deinterlacer -> noise filter -> reframe, two calls: the deinterlacer's history and the filter's state cross the
    call boundary at the INPUT geometry"""
    fmt, dn = A.SUBSAMP_422, (24, 24)
    clips = [DI.gen_interlaced(IW, IH, fmt, F, 0x1E0 + s, 1) for s in range(S)]            # F input frames = 2 F pictures
    raws, f = _uyvy(clips, IW, IH, fmt)
    den = [D.denoise_clip(DI.deint_clip(c, IW, IH, fmt, DI.FIELD, 1), IW, IH, fmt, *dn)[0] for c in clips]
    cut = D.denoise_clip(DI.deint_clip(clips[0][F // 2:], IW, IH, fmt, DI.FIELD, 1), IW, IH, fmt, *dn)[0]
    assert not np.array_equal(den[0][F:], cut)           # (the second call's history and state matter)
    framed = [R.reframe_clip(c, RF, fmt) for c in den]
    want = [oracle(("all", s), framed[s], OW, OH, fmt, qp=80)[0] for s in range(S)]
    make = lambda: pkg.Batch(pkg.make_encoder_cfg(OW, OH, fmt, **dict(CRF, qp=80)), S, F)
    assert fed_framed(pkg, make, framed) == want
    calls = calls_of(raws, F // 2)
    assert len(calls) == 2
    for form in ("host", "device"):
        b = make()
        try:
            b.set_source_reframe(cs(pkg, RF))
            b.set_source_format(pkg.PixFormat(f["layout"], f["depth"], f["msb"], f["pitch"], f["frame_bytes"]))
            b.set_source_deinterlace(pkg.Deint(DI.FIELD, 1))
            b.set_source_denoise(pkg.Denoise(*dn))
            got = run(b, calls, form, pipelined=form == "host")
        finally:
            b.close()
        assert got == want, form


# ---- resolution ladder: a 4:3 input pillarboxed onto a 2:1 canvas ----
LW, LH, CW, CH = 128, 96, 192, 96
LRF = R.rf(LW, LH, (0, 0, LW, LH), (CW, CH), (32, 0))
GEOMS = [(CW, CH, 80), (96, 48, 70)]


def ladder_want(fmt):
    key = ("lw", fmt)
    if key not in _cache:
        clips = sources(fmt, LW, LH)
        framed = [R.reframe_clip(c, LRF, fmt) for c in clips]
        want = []
        for s, clip in enumerate(framed):
            for gw, gh, qp in GEOMS:
                sc = clip if (gw, gh) == (CW, CH) else Z.scale_clip(clip, CW, CH, fmt, gw, gh, Z.CUBIC)
                want.append(oracle(("r", s, gw), sc, gw, gh, fmt, qp=qp)[0])
        _cache[key] = clips, framed, want
    return _cache[key]


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


def test_resolution_ladder(pkg, orc):
    fmt = A.SUBSAMP_420
    clips, framed, want = ladder_want(fmt)
    geoms = lambda: [(gw, gh, [pkg.make_encoder_cfg(gw, gh, fmt, **dict(CRF, qp=qp))]) for gw, gh, qp in GEOMS]
    # the ladder fed the framed clip: packets and source-resolution figures to compare with
    b = pkg.ResLadder(CW, CH, fmt, geoms(), S, F, Z.CUBIC)
    try:
        b.src_quality_enable(sse=True, ssim=True, filt=Z.CUBIC)
        base, bsse, bssim = ladder_run(b, calls_of(framed, F), "host")
    finally:
        b.close()
    assert base == want
    for form in ("host", "held"):
        b = pkg.ResLadder(LW, LH, fmt, geoms(), S, F, Z.CUBIC, reframe=cs(pkg, LRF))
        try:
            assert (b.width, b.height) == (CW, CH) and b.frame_bytes == A.frame_bytes(LW, LH, fmt)
            b.src_quality_enable(sse=True, ssim=True, filt=Z.CUBIC)
            got, xsse, xssim = ladder_run(b, calls_of(clips, F), form)
            up = b.uploads()
        finally:
            b.close()
        assert got == want, form
        assert np.array_equal(xsse, bsse) and np.array_equal(xssim, bssim), form
        assert up == ((2 * S * F * A.frame_bytes(LW, LH, fmt), 2) if form == "host" else (0, 0))


def test_resolution_ladder_passes_act_in_front_of_the_reframe(pkg, orc):
    fmt, dn = A.SUBSAMP_420, (24, 24)
    clips = sources(fmt, LW, LH)
    framed = [R.reframe_clip(D.denoise_clip(c, LW, LH, fmt, *dn)[0], LRF, fmt) for c in clips]
    want = [oracle(("rd", s), framed[s], CW, CH, fmt, qp=80)[0] for s in range(S)]
    b = pkg.ResLadder(LW, LH, fmt, [(CW, CH, [pkg.make_encoder_cfg(CW, CH, fmt, **dict(CRF, qp=80))])], S, F, Z.CUBIC, reframe=cs(pkg, LRF))
    try:
        b.set_denoise(pkg.Denoise(*dn))
        got = [b""] * b.nstreams
        for c in calls_of(clips, F):
            got[:] = [x + bytes(p) for x, p in zip(got, b.encode(c))]
    finally:
        b.close()
    assert got == want


# ---- errors and the feature off --------------------------------------------------------------------------------------------------
def test_error_contract(pkg, orc):
    fmt = A.SUBSAMP_420
    L = pkg.lib()
    clips = sources(fmt)
    framed = [R.reframe_clip(c, RF, fmt) for c in clips]
    want = oracle(("b", 0), framed[0], OW, OH, fmt, qp=80)[0]
    plain = oracle(("p", 0), sources(fmt, OW, OH)[0], OW, OH, fmt, qp=80)[0]
    cfg = pkg.make_encoder_cfg(OW, OH, fmt, **dict(CRF, qp=80))
    calls = calls_of(clips[:1], F)
    good = cs(pkg, RF)
    bads = [cs(pkg, dict(RF, x=7)), cs(pkg, dict(RF, w=65)), cs(pkg, dict(RF, dst_x=48)), cs(pkg, dict(RF, out_w=OW + 16)),
            cs(pkg, dict(RF, out_h=OH - 16, dst_y=0)), cs(pkg, dict(RF, in_w=0))]
    res = cs(pkg, RF)
    res.reserved = 1
    bads.append(res)
    b = pkg.Batch(cfg, 1, F)
    try:
        # an invalid struct, a canvas that is not the batch's geometry: refused, and the next submit behaves as before (nothing set)
        for bad in bads:
            assert L.dsv1_batch_set_source_reframe(b.h, C.byref(bad)) == DSVG_ERR_ARG
        assert not L.dsv1_batch_has_source_lane(b.h)
        p1 = bytes(b.encode(calls_of(sources(fmt, OW, OH)[:1], F)[0])[0])
        assert p1 and plain.startswith(p1)
        # a pass already set
        b.set_source_denoise(pkg.Denoise(24, 24))
        assert L.dsv1_batch_set_source_reframe(b.h, C.byref(good)) == DSVG_ERR_ARG
        b.set_source_denoise(None)
        b.set_source_deinterlace(pkg.Deint(DI.FRAME, 1))
        assert L.dsv1_batch_set_source_reframe(b.h, C.byref(good)) == DSVG_ERR_ARG
        b.set_source_deinterlace(None)
        b.set_source_format(pkg.PixFormat(PF.UYVY), src_subsamp=A.SUBSAMP_422)
        assert L.dsv1_batch_set_source_reframe(b.h, C.byref(good)) == DSVG_ERR_ARG
        b.set_source_format(None)
        # a clip staged
        pin = b.pinned((1, F, A.frame_bytes(OW, OH, fmt)))
        pin[...] = calls_of(sources(fmt, OW, OH)[:1], F)[1]
        assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == 0
        assert L.dsv1_batch_set_source_reframe(b.h, C.byref(good)) == DSVG_ERR_ARG
        b.submit(pin)
        assert L.dsv1_batch_set_source_reframe(b.h, C.byref(good)) == DSVG_ERR_ARG                              # a batch in flight
        assert p1 + bytes(b.collect()[0]) == plain       # every refusal left the batch as it was: it codes the clips themselves
        assert not L.dsv1_batch_has_source_lane(b.h)
    finally:
        b.close()
    b = pkg.Batch(cfg, 1, F)
    try:
        b.set_source_reframe(good)
        assert L.dsv1_batch_has_source_lane(b.h)
        pin = b.pinned(calls[0].shape)
        pin[...] = calls[0]
        assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == DSVG_ERR_ARG                                          # stage is refused while set
        b.submit(pin)
        for x in [None, good] + bads:                                                                            # in flight, invalid: as it was
            assert L.dsv1_batch_set_source_reframe(b.h, C.byref(x) if x is not None else None) == DSVG_ERR_ARG
        first = b.collect()[0]
        for bad in bads:
            assert L.dsv1_batch_set_source_reframe(b.h, C.byref(bad)) == DSVG_ERR_ARG
        b.set_source_denoise(pkg.Denoise(24, 24))                                                                 # set after it: fine; then it is locked
        assert L.dsv1_batch_set_source_reframe(b.h, None) == DSVG_ERR_ARG
        b.set_source_denoise(None)
        assert bytes(first) + bytes(b.encode(calls[1])[0]) == want
    finally:
        b.close()
    # the resolution ladder's open
    meta = pkg.Meta()
    meta.width, meta.height, meta.subsamp = LW, LH, fmt
    h = C.c_void_p(None)

    def open_(m, rfr, pf, rgb, gw, gh):
        enc = (pkg.Encoder * 1)(pkg.make_encoder_cfg(gw, gh, fmt, **dict(CRF, qp=80)))
        rr = (pkg.ResRung * 1)(pkg.ResRung(gw, gh, 1, enc))
        return L.dsv1_resladder_open_reframed(C.byref(h), C.byref(m), C.byref(rfr), pf, fmt, rgb, rr, 1, 0, 1, F, Z.CUBIC)

    other = pkg.Meta()
    other.width, other.height, other.subsamp = CW, CH, fmt
    assert open_(other, cs(pkg, LRF), None, None, CW, CH) == DSVG_ERR_ARG and h.value is None                    # src is not in_w x in_h
    assert open_(meta, cs(pkg, LRF), C.byref(pkg.PixFormat()), C.byref(pkg.RgbFormat()), CW, CH) == DSVG_ERR_ARG and h.value is None
    # a rung larger than the canvas is refused although it is smaller than the input
    crop = cs(pkg, R.rf(LW, LH, (16, 8, 64, 48), (64, 48)))
    assert open_(meta, crop, None, None, 96, 64) == DSVG_ERR_ARG and h.value is None
    assert open_(meta, crop, None, None, 64, 48) == 0 and h.value is not None
    L.dsv1_resladder_close(h)


def test_feature_off(pkg, orc):
    """a batch and a resolution ladder that never call the setter, and a batch that set and cleared it (or set the identity), write the
    oracle's streams of the clip itself; a cleared chain holds no lane"""
    fmt = A.SUBSAMP_420
    L = pkg.lib()
    clips = sources(fmt, OW, OH)
    want = [oracle(("off", s), clips[s], OW, OH, fmt, qp=80)[0] for s in range(S)]
    calls = calls_of(clips, F)
    cfg = pkg.make_encoder_cfg(OW, OH, fmt, **dict(CRF, qp=80))
    for mode in ("never", "cleared", "identity"):
        b = pkg.Batch(cfg, S, F)
        try:
            if mode == "cleared":
                b.set_source_reframe(cs(pkg, RF))
                assert L.dsv1_batch_has_source_lane(b.h)
                b.set_source_reframe(None)
            if mode == "identity":
                b.set_source_reframe(cs(pkg, R.rf(OW, OH, (0, 0, OW, OH), (OW, OH))))
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
    lclips = sources(fmt, CW, CH)
    lwant = []
    for s in range(S):
        for gw, gh, qp in GEOMS:
            sc = lclips[s] if (gw, gh) == (CW, CH) else Z.scale_clip(lclips[s], CW, CH, fmt, gw, gh, Z.CUBIC)
            lwant.append(oracle(("loff", s, gw), sc, gw, gh, fmt, qp=qp)[0])
    r = pkg.ResLadder(CW, CH, fmt, [(gw, gh, [pkg.make_encoder_cfg(gw, gh, fmt, **dict(CRF, qp=qp))]) for gw, gh, qp in GEOMS], S, F, Z.CUBIC)
    try:
        got = [b""] * r.nstreams
        for c in calls_of(lclips, F):
            got[:] = [x + bytes(p) for x, p in zip(got, r.encode(c))]
    finally:
        r.close()
    assert got == lwant
