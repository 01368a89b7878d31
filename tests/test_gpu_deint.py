"""Deinterlacing on the GPU (include/dsv1_api.h, Deinterlacing; csrc/k_deint.hip): dsv1_deinterlace_clip equals the numpy statement
tests/_deint.py byte for byte on the 16-byte path and on the byte path, touching nothing around its buffers; batches, quality
ladders, chain mode and resolution ladders with a deinterlacer set write the streams the oracle writes for the numpy-deinterlaced
whole clip -- the history crosses the call boundary -- and measure against it."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import _deint as D
import _pixfmt as PF
import _resample as RS
import _rgb as RG
import _scale as Z

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2
CRF = dict(gop=4, rc_mode_cli=1, scd=1)
W, H, S, F = 352, 288, 2, 4


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


def test_geometry_list_reaches_both_paths():
    """from the geometry alone: a case whose every plane is on the 16-byte path, cases with none, and mixed ones"""
    fast = {(w, h): D.planes_fast(w, h, fmt) for w, h, fmt in D.GPU_GEOMS}
    assert fast[(352, 288)] == [True, True, True] and 352 // 16 > 2 and 176 // 16 > 2       # (items between a row's first and last)
    assert fast[(250, 130)] == [False] * 3 and fast[(35, 19)] == [False] * 3 and fast[(36, 20)] == [False] * 3
    assert fast[(48, 18)] == [True, False, False]         # 24-byte chroma rows; luma: three items a row, one of them inside
    assert fast[(64, 3)] == [True, True, True]            # 64 and 32-byte rows, three rows: both row rules in one run
    assert fast[(16, 2)] == [True, False, False]          # chroma of one row
    assert fast[(1, 1)] == [False] * 3
    assert A.chroma_dims(36, 20, A.SUBSAMP_411)[0] < 16 and 36 % 16 and 48 % 16 == 0       # tails: a row of one short item, a tail item, none


@pytest.mark.parametrize("w,h,fmt", D.GPU_GEOMS)
def test_deinterlace_clip_equals_numpy(pkg, mem, w, h, fmt):
    n, fb = D.GPU_FRAMES, A.frame_bytes(w, h, fmt)
    ncases = 0
    for mode in (D.FRAME, D.FIELD):
        for tff in (0, 1):
            frames, before = D.gpu_case(w, h, fmt, tff)  # (tests/test_deint_host.py counts what exactly these reach)
            di = pkg.Deint(mode, tff)
            for prev in (None, before):
                want = D.deint_clip(frames, w, h, fmt, mode, tff, prev=prev)
                got = pkg.deinterlace_clip(frames, w, h, fmt, di, prev=prev)
                assert got.shape == want.shape == (D.out_frames(mode, n), fb)
                A.assert_same("host mode %d tff %d prev %s" % (mode, tff, prev is not None), got, want)
                # device memory: the three buffers exactly as long as their frames inside larger allocations of a known pattern,
                # 16-byte aligned (the 16-byte path where the geometry allows it) and not (the byte path for every geometry)
                for soff, doff in ((4096, 4096), (4096 + 3, 4096 + 16)):
                    big_s = np.full(soff + n * fb + 4096, 0xC3, dtype=np.uint8)
                    big_s[soff:soff + n * fb] = frames.reshape(-1)
                    big_p = np.full(soff + fb + 4096, 0x5A, dtype=np.uint8)
                    big_p[soff:soff + fb] = before
                    big_d = np.full(doff + want.size + 4096, 0x3C, dtype=np.uint8)
                    ps, pp, pd = mem.alloc(big_s), mem.alloc(big_p), mem.alloc(big_d)
                    pkg.deinterlace_clip(C.c_void_p(ps.value + soff), w, h, fmt, di, prev=C.c_void_p(pp.value + soff) if prev is not None else None,
                                         n=n, out=C.c_void_p(pd.value + doff))
                    after = mem.read(pd, big_d.size)
                    assert (after[:doff] == 0x3C).all() and (after[doff + want.size:] == 0x3C).all(), "written outside the destination"
                    A.assert_same("device mode %d tff %d prev %s offsets %d %d" % (mode, tff, prev is not None, soff, doff),
                                  after[doff:doff + want.size].reshape(want.shape), want)
                    assert np.array_equal(mem.read(ps, big_s.size), big_s) and np.array_equal(mem.read(pp, big_p.size), big_p)
                    ncases += 1
    assert ncases == 16


# ---- sessions ------------------------------------------------------------------------------------------------------------------
_cache = {}


def sources(fmt, mode, tff=1):
    """S interlaced sources that make 2 F pictures each, their numpy-deinterlaced whole clips"""
    key = ("src", fmt, mode, tff)
    if key not in _cache:
        n = 2 * F // (2 if mode == D.FIELD else 1)
        clips = [D.gen_interlaced(W, H, fmt, n, 0x1E0 + s, tff) for s in range(S)]
        _cache[key] = clips, [D.deint_clip(c, W, H, fmt, mode, tff) for c in clips]
    return _cache[key]


def oracle(key, clip, w, h, fmt, **rate):
    """(stream, reconstructions) the oracle makes of a clip, once per key"""
    if key not in _cache:
        _cache[key] = A.orc_encode(clip, A.orc_cfg(w, h, fmt, **dict(CRF, **rate)), want_recon=True, eos=False)
    return _cache[key]


def calls_of(clips, per_call):
    """[S, frames of a call, bytes] per call"""
    return [np.ascontiguousarray(np.stack([c[k * per_call:(k + 1) * per_call] for c in clips])) for k in range(clips[0].shape[0] // per_call)]


def run(b, calls, form, pipelined=True, sse=False):
    """submit / collect the calls -> (streams, [sse per call])"""
    dev = form != "host"
    junk = np.full(calls[0].size, 0xA5, dtype=np.uint8)
    ins = [b.upload(c) for c in calls] if dev else calls
    got, figs = [b""] * b.nstreams, []

    def submit(c):
        b.submit(c, on_device=dev, held=form == "held")
        if form == "device":                             # a plain device clip is the caller's again when submit returns
            assert b.L.dsvg_dev_upload(b.ctx, c, junk.ctypes.data, junk.nbytes) == 0

    def take():
        part = b.collect()
        got[:] = [x + bytes(p) for x, p in zip(got, part)]
        if sse:
            figs.append(b.sse())

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
    return got, figs


def plane_sse(a, b, w, h, fmt):
    out = np.zeros(3, dtype=np.uint64)
    for p, (x, y) in enumerate(zip(RS.planes(a, w, h, fmt), RS.planes(b, w, h, fmt))):
        d = x.astype(np.int64) - y.astype(np.int64)
        out[p] = int((d * d).sum())
    return out


@pytest.mark.parametrize("mode", [D.FRAME, D.FIELD], ids=["frame", "field"])
def test_batch(pkg, orc, mode):
    fmt = A.SUBSAMP_420
    clips, deint = sources(fmt, mode)
    want = [oracle(("b", mode, s), deint[s], W, H, fmt, qp=80) for s in range(S)]
    calls = calls_of(clips, F // (2 if mode == D.FIELD else 1))
    assert len(calls) == 2
    cfg = pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80))
    for form in ("host", "device", "held"):
        b = pkg.Batch(cfg, S, F)
        try:
            b.set_source_deinterlace(pkg.Deint(mode, 1))
            b.sse_enable()
            got, figs = run(b, calls, form, pipelined=form != "device", sse=True)
        finally:
            b.close()
        sse = np.concatenate(figs, axis=1)
        for s in range(S):
            assert got[s] == want[s][0], "%s: source %d: not the oracle's stream of the deinterlaced clip" % (form, s)
            e = np.stack([plane_sse(deint[s][t], r, W, H, fmt) for t, r in enumerate(want[s][1])])
            assert np.array_equal(sse[s], e), "%s: source %d: SSE is not against the deinterlaced source" % (form, s)


def test_reset_makes_the_next_frame_a_first_frame(pkg, orc):
    fmt, mode = A.SUBSAMP_420, D.FRAME
    clips, _ = sources(fmt, mode)
    # source 1 is cut between the calls, source 0 runs on
    deint = [D.deint_clip(clips[0], W, H, fmt, mode, 1),
             np.concatenate([D.deint_clip(clips[1][:F], W, H, fmt, mode, 1), D.deint_clip(clips[1][F:], W, H, fmt, mode, 1)])]
    assert not np.array_equal(deint[1], sources(fmt, mode)[1][1])
    want = [oracle(("reset", s), deint[s], W, H, fmt, qp=80)[0] for s in range(S)]
    calls = calls_of(clips, F)
    b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
    try:
        b.set_source_deinterlace(pkg.Deint(mode, 1))
        first = b.encode(calls[0])
        b.deinterlace_reset(1)
        second = b.encode(calls[1])
    finally:
        b.close()
    for s in range(S):
        assert first[s] + second[s] == want[s], s


def test_quality_ladder_and_chain_mode(pkg, orc):
    fmt = A.SUBSAMP_420
    qps = (60, 90)
    for mode in (D.FRAME, D.FIELD):
        clips, deint = sources(fmt, mode)
        calls = calls_of(clips, F // (2 if mode == D.FIELD else 1))
        rungs = [pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=q)) for q in qps]
        for form in ("host", "device", "held"):
            b = pkg.Ladder(rungs, S, F)
            try:
                b.set_source_deinterlace(pkg.Deint(mode, 1))
                got, _ = run(b, calls, form, pipelined=form != "device")
            finally:
                b.close()
            for s in range(S):
                for r, q in enumerate(qps):
                    assert got[s * 2 + r] == oracle(("l", mode, s, q), deint[s], W, H, fmt, qp=q)[0], (mode, form, s, r)
        # chain mode: one stream, consecutive frames
        want = oracle(("c", mode), deint[0], W, H, fmt, qp=75)[0]
        cfg = pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=75))
        for form in ("host", "device", "held"):
            b = pkg.Batch(cfg, 1, F, chains=2)
            try:
                b.set_source_deinterlace(pkg.Deint(mode, 1))
                got, _ = run(b, [c[:1] for c in calls], form, pipelined=False)
            finally:
                b.close()
            assert got[0] == want, (mode, form)


@pytest.mark.parametrize("mode", [D.FRAME, D.FIELD], ids=["frame", "field"])
def test_behind_a_uyvy_source(pkg, orc, mode):
    fmt = A.SUBSAMP_422
    clips, deint = sources(fmt, mode)
    f = PF.pf(PF.UYVY)
    raws = [PF.pack(c.astype(np.uint32), f, W, H, fmt, np.random.default_rng(s)).reshape(c.shape[0], -1) for s, c in enumerate(clips)]
    for r, c in zip(raws, clips):
        assert np.array_equal(PF.convert(r.reshape(-1), f, W, H, fmt, c.shape[0]), c)
    want = [oracle(("u", mode, s), deint[s], W, H, fmt, qp=80)[0] for s in range(S)]
    calls = calls_of(raws, F // (2 if mode == D.FIELD else 1))
    for form in ("host", "device"):
        b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
        try:
            b.set_source_format(pkg.PixFormat(f["layout"], f["depth"], f["msb"], f["pitch"], f["frame_bytes"]))
            b.set_source_deinterlace(pkg.Deint(mode, 1))
            got, _ = run(b, calls, form)
        finally:
            b.close()
        assert got == want, form


def test_behind_an_rgb_source(pkg, orc):
    fmt, mode, n = A.SUBSAMP_420, D.FIELD, F
    f = RG.rf(RG.BGRA, RG.BT709, 0)
    raws, deint = [], []
    for s in range(S):
        rgb = D.gen_interlaced(W, H, A.SUBSAMP_444, n, 0x2C0 + s)
        R, G, B = (rgb[:, k * W * H:(k + 1) * W * H].reshape(n, H, W) for k in range(3))
        raw = RG.pack(R, G, B, f, W, H, np.random.default_rng(s))
        raws.append(raw.reshape(n, -1))
        deint.append(D.deint_clip(RG.import_(raw, f, W, H, fmt, n), W, H, fmt, mode, 1))
    want = [oracle(("rgb", s), deint[s], W, H, fmt, qp=80)[0] for s in range(S)]
    calls = calls_of(raws, F // 2)
    for form in ("host", "held"):
        b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
        try:
            b.set_source_deinterlace(pkg.Deint(mode, 1))           # (either order of the two setters)
            b.set_source_rgb(pkg.RgbFormat(f["order"], f["matrix"], f["full"], f["upsample"], f["pitch"], f["frame_bytes"]))
            got, _ = run(b, calls, form)
        finally:
            b.close()
        assert got == want, form


@pytest.mark.parametrize("mode,form", [(D.FRAME, "host"), (D.FIELD, "device"), (D.FIELD, "held")])
def test_resolution_ladder(pkg, orc, mode, form):
    fmt = A.SUBSAMP_420
    geoms = [(W, H, [dict(qp=80)]), (176, 144, [dict(qp=70)])]
    clips, deint = sources(fmt, mode)
    want = []
    for s, clip in enumerate(deint):
        for gw, gh, rates in geoms:
            sc = clip if (gw, gh) == (W, H) else Z.scale_clip(clip, W, H, fmt, gw, gh, Z.CUBIC)
            for rate in rates:
                data, recs = oracle(("r", mode, s, gw, rate["qp"]), sc, gw, gh, fmt, **rate)
                want.append((data, np.stack([RS.src_quality(clip[t], r, W, H, gw, gh, fmt, Z.CUBIC)[0] for t, r in enumerate(recs)])))
    b = pkg.ResLadder(W, H, fmt, [(gw, gh, [pkg.make_encoder_cfg(gw, gh, fmt, **dict(CRF, **r)) for r in rates]) for gw, gh, rates in geoms],
                      S, F, Z.CUBIC)
    try:
        b.set_deinterlace(pkg.Deint(mode, 1))
        b.src_quality_enable(sse=True, ssim=False, filt=Z.CUBIC)
        calls = calls_of(clips, b.in_frames)
        dev = form != "host"
        junk = np.full(calls[0].size, 0x5A, dtype=np.uint8)
        ins = [b.upload(c) for c in calls] if dev else calls
        got, xs = [b""] * b.nstreams, []
        for c in ins:
            b.submit(c, on_device=dev, held=form == "held")
            if form == "device":
                assert b.L.dsvg_dev_upload(b.ctx, c, junk.ctypes.data, junk.nbytes) == 0
        for _ in ins:
            got[:] = [x + bytes(p) for x, p in zip(got, b.collect())]
            xs.append(b.src_sse())
    finally:
        b.close()
    xs = np.concatenate(xs, axis=1)
    for k, (data, xsse) in enumerate(want):
        assert got[k] == data, "output stream %d: packets differ from the oracle's" % k
        assert np.array_equal(xs[k], xsse), "output stream %d: source-resolution SSE differs" % k


def test_error_contract(pkg, orc):
    fmt, mode = A.SUBSAMP_420, D.FRAME
    L = pkg.lib()
    clips, deint = sources(fmt, mode)
    want = oracle(("b", mode, 0), deint[0], W, H, fmt, qp=80)[0]
    cfg = pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80))
    calls = calls_of(clips[:1], F)
    odd = pkg.Batch(cfg, 1, 3)
    b = pkg.Batch(cfg, 1, F)
    r = pkg.ResLadder(W, H, fmt, [(176, 144, [pkg.make_encoder_cfg(176, 144, fmt, **dict(CRF, qp=70))])], 1, 3, Z.CUBIC)
    try:
        assert L.dsv1_batch_set_source_deinterlace(odd.h, C.byref(pkg.Deint(D.FIELD, 1))) == DSVG_ERR_ARG      # odd frames_per_call
        odd.set_source_deinterlace(pkg.Deint(D.FRAME, 1))
        assert L.dsv1_resladder_set_deinterlace(r.h, C.byref(pkg.Deint(D.FIELD, 0))) == DSVG_ERR_ARG
        assert L.dsv1_resladder_set_deinterlace(r.h, C.byref(pkg.Deint(0, 2))) == DSVG_ERR_ARG
        assert L.dsv1_resladder_deinterlace_reset(r.h, -1) == DSVG_ERR_ARG                                     # none set
        r.set_deinterlace(pkg.Deint(D.FRAME, 0))
        assert L.dsv1_resladder_deinterlace_reset(r.h, 1) == DSVG_ERR_ARG                                      # one source
        r.deinterlace_reset(0)
        # the resolution ladder with a call in flight: setter and reset are refused, the setting and the history stay
        rclip = calls[0][:, :3]
        rwant = oracle(("rerr",), Z.scale_clip(D.deint_clip(np.concatenate([rclip[0], rclip[0]]), W, H, fmt, D.FRAME, 0), W, H, fmt, 176, 144, Z.CUBIC),
                       176, 144, fmt, qp=70)[0]
        r.submit(rclip)
        assert L.dsv1_resladder_set_deinterlace(r.h, None) == DSVG_ERR_ARG
        assert L.dsv1_resladder_set_deinterlace(r.h, C.byref(pkg.Deint(D.FRAME, 1))) == DSVG_ERR_ARG
        assert L.dsv1_resladder_deinterlace_reset(r.h, 0) == DSVG_ERR_ARG and L.dsv1_resladder_deinterlace_reset(r.h, -1) == DSVG_ERR_ARG
        rfirst = r.collect()[0]
        assert bytes(rfirst) + bytes(r.encode(rclip)[0]) == rwant
        assert L.dsv1_batch_deinterlace_reset(b.h, -1) == DSVG_ERR_ARG                                         # none set
        b.set_source_deinterlace(pkg.Deint(mode, 1))
        for bad in (pkg.Deint(2, 1), pkg.Deint(-1, 0), pkg.Deint(0, 2), pkg.Deint(1, -1)):
            assert L.dsv1_batch_set_source_deinterlace(b.h, C.byref(bad)) == DSVG_ERR_ARG
        assert L.dsv1_batch_deinterlace_reset(b.h, 1) == DSVG_ERR_ARG and L.dsv1_batch_deinterlace_reset(b.h, -2) == DSVG_ERR_ARG
        pin = b.pinned(calls[0].shape)
        pin[...] = calls[0]
        assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == DSVG_ERR_ARG
        with pytest.raises(ValueError):
            b.submit(calls[0][:, :F // 2])
        b.submit(pin)
        assert L.dsv1_batch_set_source_deinterlace(b.h, None) == DSVG_ERR_ARG                                  # a batch in flight
        assert L.dsv1_batch_set_source_deinterlace(b.h, C.byref(pkg.Deint(D.FIELD, 1))) == DSVG_ERR_ARG
        assert L.dsv1_batch_deinterlace_reset(b.h, 0) == DSVG_ERR_ARG
        first = b.collect()[0]
        # every refusal left the setting, and the history, as they were: the stream goes on as the uncut clip's
        second = b.encode(calls[1])[0]
        assert first + second == want
        b.set_source_deinterlace(None)
        assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == 0
        b.submit(pin)
        b.collect()
    finally:
        odd.close()
        b.close()
        r.close()
