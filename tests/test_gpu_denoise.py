"""Temporal noise reduction on the GPU (include/dsv1_api.h, Temporal noise reduction; csrc/k_denoise.hip): dsv1_denoise_clip equals the
numpy statement tests/_denoise.py byte for byte, pictures and state, on the 16-byte path and on the byte path, touching nothing around
its buffers; batches, quality ladders, chain mode and resolution ladders with a filter set write the streams the oracle writes for
the numpy-filtered whole clip -- the state crosses the call boundary -- and measure against it."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import _deint as DI
import _denoise as D
import _pixfmt as PF
import _resample as RS
import _rgb as RG
import _scale as Z

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2
CRF = dict(gop=4, rc_mode_cli=1, scd=1)
W, H, S, F = 352, 288, 2, 4
DN = (24, 24)


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
    assert fast[(352, 288)] == [True, True, True] and 352 // 16 > 2 and 176 // 16 > 2 and 288 % 4 == 0 and 144 % 4 == 0
    assert fast[(250, 130)] == [False] * 3 and fast[(35, 19)] == [False] * 3 and fast[(36, 20)] == [False] * 3
    assert fast[(64, 3)] == [True, True, True]            # three rows: an item whose last row is outside the plane, both row clamps in one item
    assert fast[(16, 2)] == [True, False, False]          # chroma of one row of 8: the byte path with a tail and both clamps on every sample
    assert fast[(1, 1)] == [False] * 3
    assert A.chroma_dims(36, 20, A.SUBSAMP_411)[0] < 16 and 36 % 16 and 250 % 16        # tails: a row of one short item, a tail item
    assert {s for s in D.GPU_STRENGTHS if 0 in s} == {(40, 0), (0, 16)}                  # the copy on either kind of plane


@pytest.mark.parametrize("w,h,fmt", D.GPU_GEOMS)
def test_denoise_clip_equals_numpy(pkg, mem, w, h, fmt):
    n, fb = D.GPU_FRAMES, A.frame_bytes(w, h, fmt)
    sb = D.state_bytes(w, h, fmt)
    frames, before = D.gpu_case(w, h, fmt)               # (tests/test_denoise_host.py counts what exactly these reach)
    ncases = 0
    for luma, chroma in D.GPU_STRENGTHS:
        dn = pkg.Denoise(luma, chroma)
        _, left = D.denoise_clip(before[None], w, h, fmt, luma, chroma)
        for state in (None, left):
            what = "%d/%d state %s" % (luma, chroma, state is not None)
            want, wstate = D.denoise_clip(frames, w, h, fmt, luma, chroma, state=state)
            got, gstate = pkg.denoise_clip(frames, w, h, fmt, dn, state=state)
            A.assert_same("host " + what, got, want)
            A.assert_same("host state " + what, gstate, wstate)
            # device memory: the buffers exactly as long as their contents inside larger allocations of a known pattern, 16-byte
            # aligned (the 16-byte path where the geometry allows it) and not (the byte path for every geometry)
            for soff, doff in ((4096, 4096), (4096 + 3, 4096 + 16)):
                big_s = np.full(soff + n * fb + 4096, 0xC3, dtype=np.uint8)
                big_s[soff:soff + n * fb] = frames.reshape(-1)
                big_i = np.full(soff + sb + 4096, 0x5A, dtype=np.uint8)
                big_i[soff:soff + sb] = left
                big_d = np.full(doff + want.size + 4096, 0x3C, dtype=np.uint8)
                big_o = np.full(doff + sb + 4096, 0x69, dtype=np.uint8)
                ps, pi, pd, po = mem.alloc(big_s), mem.alloc(big_i), mem.alloc(big_d), mem.alloc(big_o)
                pkg.denoise_clip(C.c_void_p(ps.value + soff), w, h, fmt, dn, state=C.c_void_p(pi.value + soff) if state is not None else None,
                                 n=n, out=C.c_void_p(pd.value + doff), state_out=C.c_void_p(po.value + doff))
                after, safter = mem.read(pd, big_d.size), mem.read(po, big_o.size)
                assert (after[:doff] == 0x3C).all() and (after[doff + want.size:] == 0x3C).all(), "written outside the destination"
                assert (safter[:doff] == 0x69).all() and (safter[doff + sb:] == 0x69).all(), "written outside the state"
                A.assert_same("device %s offsets %d %d" % (what, soff, doff), after[doff:doff + want.size].reshape(want.shape), want)
                A.assert_same("device state %s offsets %d %d" % (what, soff, doff), safter[doff:doff + sb], wstate)
                assert np.array_equal(mem.read(ps, big_s.size), big_s) and np.array_equal(mem.read(pi, big_i.size), big_i)
                ncases += 1
    assert ncases == 16


def test_cut_invariance_on_the_device(pkg):
    w, h, fmt = D.GPU_GEOMS[0]
    frames, _ = D.gpu_case(w, h, fmt)
    dn = pkg.Denoise(*DN)
    whole, end = pkg.denoise_clip(frames, w, h, fmt, dn)
    want, wend = D.denoise_clip(frames, w, h, fmt, *DN)
    A.assert_same("whole", whole, want)
    for cut in (1, 2):
        head, state = pkg.denoise_clip(frames[:cut], w, h, fmt, dn)
        tail, end2 = pkg.denoise_clip(frames[cut:], w, h, fmt, dn, state=state)
        A.assert_same("cut %d" % cut, np.concatenate([head, tail]), whole)
        A.assert_same("cut %d state" % cut, end2, end)
    A.assert_same("state", end, wend)


# ---- sessions ------------------------------------------------------------------------------------------------------------------
_cache = {}


def sources(fmt):
    """S noisy sources of 2 F pictures each, their numpy-filtered whole clips"""
    key = ("src", fmt)
    if key not in _cache:
        clips = [D.gen_noisy(W, H, fmt, 2 * F, 0x2E0 + s) for s in range(S)]
        _cache[key] = clips, [D.denoise_clip(c, W, H, fmt, *DN)[0] for c in clips]
    return _cache[key]


def interlaced(fmt, mode):
    """S interlaced sources that make 2 F pictures each"""
    key = ("isrc", fmt, mode)
    if key not in _cache:
        _cache[key] = [DI.gen_interlaced(W, H, fmt, 2 * F // (2 if mode == DI.FIELD else 1), 0x1E0 + s, 1) for s in range(S)]
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


def test_batch(pkg, orc):
    fmt = A.SUBSAMP_420
    clips, den = sources(fmt)
    assert not np.array_equal(den[0][F:], D.denoise_clip(clips[0][F:], W, H, fmt, *DN)[0])      # (the second call's history matters)
    want = [oracle(("b", s), den[s], W, H, fmt, qp=80) for s in range(S)]
    calls = calls_of(clips, F)
    assert len(calls) == 2
    cfg = pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80))
    for form in ("host", "device", "held"):
        b = pkg.Batch(cfg, S, F)
        try:
            b.set_source_denoise(pkg.Denoise(*DN))
            b.sse_enable()
            got, figs = run(b, calls, form, pipelined=form != "device", sse=True)
        finally:
            b.close()
        sse = np.concatenate(figs, axis=1)
        for s in range(S):
            assert got[s] == want[s][0], "%s: source %d: not the oracle's stream of the filtered clip" % (form, s)
            e = np.stack([plane_sse(den[s][t], r, W, H, fmt) for t, r in enumerate(want[s][1])])
            assert np.array_equal(sse[s], e), "%s: source %d: SSE is not against the filtered source" % (form, s)


def test_reset_makes_the_next_picture_a_first_picture(pkg, orc):
    fmt = A.SUBSAMP_420
    clips, whole = sources(fmt)
    # source 1 is cut between the calls, source 0 runs on
    den = [whole[0], np.concatenate([D.denoise_clip(clips[1][:F], W, H, fmt, *DN)[0], D.denoise_clip(clips[1][F:], W, H, fmt, *DN)[0]])]
    assert not np.array_equal(den[1], whole[1])
    want = [oracle(("b", 0), den[0], W, H, fmt, qp=80)[0], oracle(("reset", 1), den[1], W, H, fmt, qp=80)[0]]
    calls = calls_of(clips, F)
    b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
    try:
        b.set_source_denoise(pkg.Denoise(*DN))
        first = b.encode(calls[0])
        b.denoise_reset(1)
        second = b.encode(calls[1])
    finally:
        b.close()
    for s in range(S):
        assert first[s] + second[s] == want[s], s


def test_quality_ladder_and_chain_mode(pkg, orc):
    fmt = A.SUBSAMP_420
    qps = (60, 90)
    clips, den = sources(fmt)
    calls = calls_of(clips, F)
    rungs = [pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=q)) for q in qps]
    for form in ("host", "held"):
        b = pkg.Ladder(rungs, S, F)
        try:
            b.set_source_denoise(pkg.Denoise(*DN))
            got, _ = run(b, calls, form)
        finally:
            b.close()
        for s in range(S):
            for r, q in enumerate(qps):
                assert got[s * 2 + r] == oracle(("l", s, q), den[s], W, H, fmt, qp=q)[0], (form, s, r)
    # chain mode: one stream, consecutive frames
    want = oracle(("c",), den[0], W, H, fmt, qp=75)[0]
    cfg = pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=75))
    for form in ("host", "device"):
        b = pkg.Batch(cfg, 1, F, chains=2)
        try:
            b.set_source_denoise(pkg.Denoise(*DN))
            got, _ = run(b, [c[:1] for c in calls], form, pipelined=False)
        finally:
            b.close()
        assert got[0] == want, form


def test_behind_a_uyvy_source(pkg, orc):
    fmt = A.SUBSAMP_422
    clips, den = sources(fmt)
    f = PF.pf(PF.UYVY)
    raws = [PF.pack(c.astype(np.uint32), f, W, H, fmt, np.random.default_rng(s)).reshape(c.shape[0], -1) for s, c in enumerate(clips)]
    for r, c in zip(raws, clips):
        assert np.array_equal(PF.convert(r.reshape(-1), f, W, H, fmt, c.shape[0]), c)
    want = [oracle(("u", s), den[s], W, H, fmt, qp=80)[0] for s in range(S)]
    calls = calls_of(raws, F)
    for form in ("host", "device"):
        b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
        try:
            b.set_source_format(pkg.PixFormat(f["layout"], f["depth"], f["msb"], f["pitch"], f["frame_bytes"]))
            b.set_source_denoise(pkg.Denoise(*DN))
            got, _ = run(b, calls, form)
        finally:
            b.close()
        assert got == want, form


def test_behind_an_rgb_source(pkg, orc):
    fmt, n = A.SUBSAMP_420, 2 * F
    f = RG.rf(RG.BGRA, RG.BT709, 0)
    raws, den = [], []
    for s in range(S):
        rgb = D.gen_noisy(W, H, A.SUBSAMP_444, n, 0x3C0 + s)
        R, G, B = (rgb[:, k * W * H:(k + 1) * W * H].reshape(n, H, W) for k in range(3))
        raw = RG.pack(R, G, B, f, W, H, np.random.default_rng(s))
        raws.append(raw.reshape(n, -1))
        den.append(D.denoise_clip(RG.import_(raw, f, W, H, fmt, n), W, H, fmt, *DN)[0])
    want = [oracle(("rgb", s), den[s], W, H, fmt, qp=80)[0] for s in range(S)]
    calls = calls_of(raws, F)
    for form in ("host", "held"):
        b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
        try:
            b.set_source_denoise(pkg.Denoise(*DN))                 # (either order of the two setters)
            b.set_source_rgb(pkg.RgbFormat(f["order"], f["matrix"], f["full"], f["upsample"], f["pitch"], f["frame_bytes"]))
            got, _ = run(b, calls, form)
        finally:
            b.close()
        assert got == want, form


@pytest.mark.parametrize("mode", [DI.FRAME, DI.FIELD], ids=["frame", "field"])
def test_behind_the_deinterlacer(pkg, orc, mode):
    fmt = A.SUBSAMP_420
    clips = interlaced(fmt, mode)
    den = [D.denoise_clip(DI.deint_clip(c, W, H, fmt, mode, 1), W, H, fmt, *DN)[0] for c in clips]
    want = [oracle(("di", mode, s), den[s], W, H, fmt, qp=80)[0] for s in range(S)]
    per = F // (2 if mode == DI.FIELD else 1)
    calls = calls_of(clips, per)
    for form, order in (("host", 0), ("device", 1)):
        b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
        try:
            for k in (order, 1 - order):                           # (either order of the two setters)
                if k:
                    b.set_source_denoise(pkg.Denoise(*DN))
                else:
                    b.set_source_deinterlace(pkg.Deint(mode, 1))
            got, _ = run(b, calls, form)
        finally:
            b.close()
        assert got == want, form
    # changing the deinterlacer underneath forgets the filter's state (and the deinterlacer's history): both start again
    cut = [np.concatenate([D.denoise_clip(DI.deint_clip(c[:per], W, H, fmt, mode, 1), W, H, fmt, *DN)[0],
                           D.denoise_clip(DI.deint_clip(c[per:], W, H, fmt, mode, 0), W, H, fmt, *DN)[0]]) for c in clips]
    kept = [np.concatenate([D.denoise_clip(DI.deint_clip(c[:per], W, H, fmt, mode, 1), W, H, fmt, *DN)[0][:F], D.denoise_clip(
        np.concatenate([DI.deint_clip(c[:per], W, H, fmt, mode, 1), DI.deint_clip(c[per:], W, H, fmt, mode, 0)]), W, H, fmt, *DN)[0][F:]]) for c in clips]
    assert not np.array_equal(cut[0], kept[0])           # (a filter that kept its state would code other pictures)
    want = [oracle(("dicut", mode, s), cut[s], W, H, fmt, qp=80)[0] for s in range(S)]
    b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
    try:
        b.set_source_deinterlace(pkg.Deint(mode, 1))
        b.set_source_denoise(pkg.Denoise(*DN))
        first = b.encode(calls[0])
        b.set_source_deinterlace(pkg.Deint(mode, 0))
        second = b.encode(calls[1])
    finally:
        b.close()
    assert [x + y for x, y in zip(first, second)] == want


def _uyvy(clips, fmt):
    """the clips as UYVY, [n, raw frame bytes] each, and the format"""
    f = PF.pf(PF.UYVY)
    raws = [PF.pack(c.astype(np.uint32), f, W, H, fmt, np.random.default_rng(s)).reshape(c.shape[0], -1) for s, c in enumerate(clips)]
    for r, c in zip(raws, clips):
        assert np.array_equal(PF.convert(r.reshape(-1), f, W, H, fmt, c.shape[0]), c)
    return raws, f


def test_all_three_passes(pkg, orc):
    """a UYVY source -> frame-rate deinterlacer -> noise filter: a batch with host input, and a resolution ladder with one scaled and
    one same-size geometry and a plain device clip, code the oracle's streams of the clip after tests/_pixfmt.py, tests/_deint.py and
    tests/_denoise.py in that order (and tests/_scale.py for the scaled geometry)"""
    fmt = A.SUBSAMP_422
    clips = interlaced(fmt, DI.FRAME)
    raws, f = _uyvy(clips, fmt)
    den = [D.denoise_clip(DI.deint_clip(c, W, H, fmt, DI.FRAME, 1), W, H, fmt, *DN)[0] for c in clips]
    calls = calls_of(raws, F)
    assert len(calls) == 2
    pf = pkg.PixFormat(f["layout"], f["depth"], f["msb"], f["pitch"], f["frame_bytes"])
    want = [oracle(("3b", s), den[s], W, H, fmt, qp=80)[0] for s in range(S)]
    b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)
    try:
        b.set_source_format(pf)
        b.set_source_deinterlace(pkg.Deint(DI.FRAME, 1))
        b.set_source_denoise(pkg.Denoise(*DN))
        got, _ = run(b, calls, "host")
    finally:
        b.close()
    assert got == want, "batch"
    geoms = [(W, H, 80), (176, 144, 70)]
    want = [oracle(("3b", s), den[s], W, H, fmt, qp=80)[0] if gw == W else
            oracle(("3r", s), Z.scale_clip(den[s], W, H, fmt, gw, gh, Z.CUBIC), gw, gh, fmt, qp=qp)[0] for s in range(S) for gw, gh, qp in geoms]
    r = pkg.ResLadder(W, H, fmt, [(gw, gh, [pkg.make_encoder_cfg(gw, gh, fmt, **dict(CRF, qp=qp))]) for gw, gh, qp in geoms], S, F, Z.CUBIC,
                      src_format=pf)
    try:
        r.set_deinterlace(pkg.Deint(DI.FRAME, 1))
        r.set_denoise(pkg.Denoise(*DN))
        junk = np.full(calls[0].size, 0x5A, dtype=np.uint8)
        ins = [r.upload(c) for c in calls]
        got = [b""] * r.nstreams
        for c in ins:
            r.submit(c, on_device=True)
            assert r.L.dsvg_dev_upload(r.ctx, c, junk.ctypes.data, junk.nbytes) == 0    # a plain device clip is the caller's again
        for _ in ins:
            got[:] = [x + bytes(p) for x, p in zip(got, r.collect())]
    finally:
        r.close()
    for k in range(len(want)):
        assert got[k] == want[k], "resolution ladder: output stream %d" % k


def test_setters_between_batches_on_one_lane(pkg, orc):
    """One batch, every call collected before the next change; the pass sets, in turn: none, denoise, deinterlace + denoise, UYVY +
    deinterlace + denoise (two calls, deinterlace_reset(-1) / denoise_reset(-1) between them), UYVY only; then every pass cleared and
    one more call, which codes the clip's frames themselves.  The streams are the oracle's of the concatenated numpy-modelled calls.  The documented state rules make the model:
    setting the deinterlacer resets the filter's state, a newly set filter starts fresh, changing the converter resets nothing (so
    the first call behind the converter goes on from the call before, history and state: the resets come after it, at the one kind
    of call boundary where both passes are set on either side without a setter in between)."""
    fmt = A.SUBSAMP_422
    n = 7
    clips = [DI.gen_interlaced(W, H, fmt, n * F, 0x4E0 + s, 1) for s in range(S)]
    raws, f = _uyvy(clips, fmt)
    dn = lambda c, state=None: D.denoise_clip(c, W, H, fmt, *DN, state=state)
    di = lambda c, prev=None: DI.deint_clip(c, W, H, fmt, DI.FRAME, 1, prev=prev)
    model, cont = [], []
    for c in clips:
        k = [c[i * F:(i + 1) * F] for i in range(n)]
        c3, st3 = dn(di(k[2]))                           # the deinterlacer set: the filter set by the call before starts again
        c4, _ = dn(di(k[3], prev=k[2][-1]), state=st3)   # the converter set: history and state go on
        model.append(np.concatenate([k[0], dn(k[1])[0], c3, c4, dn(di(k[4]))[0], k[5], k[6]]))
        cont.append(np.concatenate([dn(k[2])[0], dn(di(k[3]))[0]]))
    # (what a filter that kept its state over the deinterlacer's setter, or passes that started again behind the converter's, would code)
    assert not np.array_equal(model[0][2 * F:3 * F], dn(di(clips[0][2 * F:3 * F]), state=dn(clips[0][F:2 * F])[1])[0])
    assert not np.array_equal(model[0][3 * F:4 * F], cont[0][F:])
    want = [oracle(("lane", s), model[s], W, H, fmt, qp=80)[0] for s in range(S)]
    pf = pkg.PixFormat(f["layout"], f["depth"], f["msb"], f["pitch"], f["frame_bytes"])
    call = lambda src, i: np.ascontiguousarray(np.stack([c[i * F:(i + 1) * F] for c in src]))
    got = [b""] * S
    b = pkg.Batch(pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80)), S, F)

    def encode(src, i):
        got[:] = [x + bytes(p) for x, p in zip(got, b.encode(call(src, i)))]

    try:
        encode(clips, 0)
        b.set_source_denoise(pkg.Denoise(*DN))
        encode(clips, 1)
        b.set_source_deinterlace(pkg.Deint(DI.FRAME, 1))
        encode(clips, 2)
        b.set_source_format(pf)
        encode(raws, 3)
        b.deinterlace_reset(-1)
        b.denoise_reset(-1)
        encode(raws, 4)
        b.set_source_deinterlace(None)
        b.set_source_denoise(None)
        encode(raws, 5)
        b.set_source_format(None)
        encode(clips, 6)
    finally:
        b.close()
    for s in range(S):                                   # (the last call, every pass cleared, included: the clip's frames themselves)
        assert got[s] == want[s], "source %d" % s


@pytest.mark.parametrize("form", ["host", "device", "held"])
def test_resolution_ladder(pkg, orc, form):
    fmt = A.SUBSAMP_420
    geoms = [(W, H, [dict(qp=80)]), (176, 144, [dict(qp=70)])]
    clips, den = sources(fmt)
    want = []
    for s, clip in enumerate(den):
        for gw, gh, rates in geoms:
            sc = clip if (gw, gh) == (W, H) else _scaled(s, clip, fmt, gw, gh)
            for rate in rates:
                data, recs = oracle(("r", s, gw, rate["qp"]) if gw != W else ("b", s), sc, gw, gh, fmt, **rate)
                key = ("rx", s, gw)
                if key not in _cache:
                    _cache[key] = np.stack([RS.src_quality(clip[t], r, W, H, gw, gh, fmt, Z.CUBIC)[0] for t, r in enumerate(recs)])
                want.append((data, _cache[key]))
    b = pkg.ResLadder(W, H, fmt, [(gw, gh, [pkg.make_encoder_cfg(gw, gh, fmt, **dict(CRF, **r)) for r in rates]) for gw, gh, rates in geoms],
                      S, F, Z.CUBIC)
    try:
        b.set_denoise(pkg.Denoise(*DN))
        b.src_quality_enable(sse=True, ssim=False, filt=Z.CUBIC)
        calls = calls_of(clips, F)
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


def _scaled(s, clip, fmt, gw, gh):
    key = ("scaled", s, gw, gh)
    if key not in _cache:
        _cache[key] = Z.scale_clip(clip, W, H, fmt, gw, gh, Z.CUBIC)
    return _cache[key]


def test_error_contract(pkg, orc):
    fmt = A.SUBSAMP_420
    L = pkg.lib()
    clips, den = sources(fmt)
    want = oracle(("b", 0), den[0], W, H, fmt, qp=80)[0]
    cfg = pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80))
    calls = calls_of(clips[:1], F)
    bads = [pkg.Denoise(-1, 4), pkg.Denoise(4, -1), pkg.Denoise(513, 4), pkg.Denoise(4, 513), pkg.Denoise(0, 0)]
    b = pkg.Batch(cfg, 1, F)
    r = pkg.ResLadder(W, H, fmt, [(176, 144, [pkg.make_encoder_cfg(176, 144, fmt, **dict(CRF, qp=70))])], 1, F, Z.CUBIC)
    try:
        for bad in bads:
            assert L.dsv1_resladder_set_denoise(r.h, C.byref(bad)) == DSVG_ERR_ARG
        assert L.dsv1_resladder_denoise_reset(r.h, -1) == DSVG_ERR_ARG                                         # none set
        r.set_denoise(pkg.Denoise(*DN))
        assert L.dsv1_resladder_denoise_reset(r.h, 1) == DSVG_ERR_ARG and L.dsv1_resladder_denoise_reset(r.h, -2) == DSVG_ERR_ARG
        r.denoise_reset(0)
        # the resolution ladder with a call in flight: setter and reset are refused, the setting and the state stay
        rwant = oracle(("r", 0, 176, 70), _scaled(0, den[0], fmt, 176, 144), 176, 144, fmt, qp=70)[0]
        r.submit(calls[0])
        assert L.dsv1_resladder_set_denoise(r.h, None) == DSVG_ERR_ARG
        assert L.dsv1_resladder_set_denoise(r.h, C.byref(pkg.Denoise(40, 40))) == DSVG_ERR_ARG
        assert L.dsv1_resladder_denoise_reset(r.h, 0) == DSVG_ERR_ARG and L.dsv1_resladder_denoise_reset(r.h, -1) == DSVG_ERR_ARG
        rfirst = r.collect()[0]
        for bad in bads:                                           # refused, and the setting is as it was
            assert L.dsv1_resladder_set_denoise(r.h, C.byref(bad)) == DSVG_ERR_ARG
        assert bytes(rfirst) + bytes(r.encode(calls[1])[0]) == rwant
        assert L.dsv1_batch_denoise_reset(b.h, -1) == DSVG_ERR_ARG                                             # none set
        for bad in bads:
            assert L.dsv1_batch_set_source_denoise(b.h, C.byref(bad)) == DSVG_ERR_ARG
        assert L.dsv1_batch_denoise_reset(b.h, -1) == DSVG_ERR_ARG                                             # still none set
        b.set_source_denoise(pkg.Denoise(*DN))
        for bad in bads:
            assert L.dsv1_batch_set_source_denoise(b.h, C.byref(bad)) == DSVG_ERR_ARG
        assert L.dsv1_batch_denoise_reset(b.h, 1) == DSVG_ERR_ARG and L.dsv1_batch_denoise_reset(b.h, -2) == DSVG_ERR_ARG
        pin = b.pinned(calls[0].shape)
        pin[...] = calls[0]
        assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == DSVG_ERR_ARG
        b.submit(pin)
        assert L.dsv1_batch_set_source_denoise(b.h, None) == DSVG_ERR_ARG                                      # a batch in flight
        assert L.dsv1_batch_set_source_denoise(b.h, C.byref(pkg.Denoise(40, 40))) == DSVG_ERR_ARG
        assert L.dsv1_batch_denoise_reset(b.h, 0) == DSVG_ERR_ARG
        first = b.collect()[0]
        # every refusal left the setting, and the state, as they were: the stream goes on as the uncut clip's
        second = b.encode(calls[1])[0]
        assert first + second == want
        b.set_source_denoise(None)
        assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == 0
        b.submit(pin)
        b.collect()
    finally:
        b.close()
        r.close()


def test_feature_off(pkg, orc):
    """a batch with no filter set -- never set, and set and cleared again -- writes the oracle's stream of the clip itself"""
    fmt = A.SUBSAMP_420
    clips, _ = sources(fmt)
    want = [oracle(("off", s), clips[s], W, H, fmt, qp=80)[0] for s in range(S)]
    calls = calls_of(clips, F)
    cfg = pkg.make_encoder_cfg(W, H, fmt, **dict(CRF, qp=80))
    for cleared in (False, True):
        b = pkg.Batch(cfg, S, F)
        try:
            if cleared:
                b.set_source_denoise(pkg.Denoise(*DN))
                b.set_source_denoise(None)
            got, _ = run(b, calls, "host")
        finally:
            b.close()
        assert got == want, cleared
