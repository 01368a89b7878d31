"""Source pixel formats on the GPU (include/dsv1_api.h dsv1_pix_format, csrc/k_pixfmt.hip): dsv1_convert_clip equals the numpy
statement tests/_pixfmt.py byte for byte over every valid format, on the 16-byte path and on the byte path, touching nothing around
its buffers; batches, quality ladders, chain mode and resolution ladders fed NV12 / P010 / YUYV / 10-bit planar clips write the
streams the oracle writes for the converted clip, and measure against it."""
import ctypes as C
import importlib
import itertools

import numpy as np
import pytest

import _cabi as A
import _pixfmt as PF
import _resample as RS
import _scale as Z
import _ssim as SS

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2
CRF = dict(gop=12, rc_mode_cli=1, scd=1)
ABR = dict(gop=12, rc_mode_cli=0, scd=1, kbps=300)


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return m


def cpf(pkg, f):
    return pkg.PixFormat(f["layout"], f["depth"], f["msb"], f["pitch"], f["frame_bytes"])


def valid_cases():
    for layout, depth, msb, fmt in itertools.product(PF.LAYOUTS, PF.DEPTHS, (0, 1), PF.SUBSAMPS):
        if (depth > 8 or not msb) and PF.valid(layout, depth, fmt):
            yield PF.pf(layout, depth, msb), fmt


def padded(f, w, h, fmt, pad=(48, 16, 80), stride_pad=256):
    """pitches and a frame stride beyond the rows, multiples of 16 or not as `pad` says"""
    lay, _, _ = PF.plane_layout(f, w, h, fmt)
    g = dict(f, pitch=tuple(lay[k][2] + pad[k] if k < len(lay) else 0 for k in range(3)))
    return dict(g, frame_bytes=PF.plane_layout(g, w, h, fmt)[1] + stride_pad)


def segments_fast(f, w, h, fmt):
    """per source plane: does every row start 16-byte aligned, source and destination (8 for a packed layout's U and V), with buffers
    that start aligned -- the kernel's rule for its 16-byte path (csrc/k_pixfmt.hip: seg_fast)"""
    lay, _, fb = PF.plane_layout(f, w, h, fmt)
    cw, ch = A.chroma_dims(w, h, fmt)
    dfb = A.frame_bytes(w, h, fmt)
    uo, vo = w * h, w * h + cw * ch
    outs = {PF.PLANAR: [[(0, w, 16)], [(uo, cw, 16)], [(vo, cw, 16)]], PF.SEMI_UV: [[(0, w, 16)], [(uo, cw, 16), (vo, cw, 16)]],
            PF.YUYV: [[(0, w, 16), (uo, cw, 8), (vo, cw, 8)]]}
    outs[PF.SEMI_VU], outs[PF.UYVY] = outs[PF.SEMI_UV], outs[PF.YUYV]
    res = []
    for (off, pitch, _, _), o in zip(lay, outs[f["layout"]]):
        res.append((fb | off | pitch) % 16 == 0 and all((dfb | doff | dp) % al == 0 for doff, dp, al in o))
    return res


def source(f, w, h, fmt, n, seed):
    """(raw clip in format f, what the device must make of it)"""
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, 1 << f["depth"], (n, A.frame_bytes(w, h, fmt)), dtype=np.uint32)
    if f["depth"] > 8:                                   # the clamp and the ties are in every clip
        vals[:, :4] = [(1 << f["depth"]) - 1, 1 << (f["depth"] - 9), (1 << (f["depth"] - 9)) - 1, (255 << (f["depth"] - 8)) - 1]
    buf = PF.pack(vals, f, w, h, fmt, rng)
    return buf, PF.convert(buf, f, w, h, fmt, n)


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


GEOMS = [(352, 288), (250, 130), (36, 20)]


def test_geometry_list_reaches_both_paths():
    """from the geometry alone: a case whose every row is on the 16-byte path, one with none, and mixed ones"""
    nv12, p010 = PF.pf(PF.SEMI_UV), PF.pf(PF.SEMI_UV, 10, 1)
    for f in (nv12, p010, PF.pf(PF.PLANAR, 10, 0)):
        assert all(segments_fast(f, 352, 288, A.SUBSAMP_420))
        assert all(segments_fast(padded(f, 352, 288, A.SUBSAMP_420), 352, 288, A.SUBSAMP_420))
        assert not any(segments_fast(f, 250, 130, A.SUBSAMP_420))
        assert not any(segments_fast(padded(f, 250, 130, A.SUBSAMP_420, pad=(5, 3, 7), stride_pad=37), 250, 130, A.SUBSAMP_420))
    assert all(segments_fast(PF.pf(PF.YUYV), 352, 288, A.SUBSAMP_422)) and not any(segments_fast(PF.pf(PF.UYVY), 250, 130, A.SUBSAMP_422))
    assert segments_fast(PF.pf(PF.PLANAR), 352, 288, A.SUBSAMP_411) == [True, False, False]      # 88-byte chroma rows
    assert A.chroma_dims(36, 20, A.SUBSAMP_411)[0] < 16 and 36 // 2 == 18                          # (36x20: chroma rows of one tail, or one step + a tail)


@pytest.mark.parametrize("w,h", GEOMS)
def test_convert_clip_equals_numpy(pkg, mem, w, h):
    ncases = 0
    for i, (f, fmt) in enumerate(valid_cases()):
        aligned_pad = padded(f, w, h, fmt)
        odd_pad = padded(f, w, h, fmt, pad=(5, 3, 7), stride_pad=37)
        for j, g in enumerate((f, aligned_pad, odd_pad)):
            n = (1, 3, 2)[j]
            buf, want = source(g, w, h, fmt, n, 1000 * i + j)
            got = pkg.convert_clip(buf, cpf(pkg, g), w, h, fmt)
            assert got.shape == want.shape
            assert np.array_equal(got, want), "host %s fmt 0x%x %dx%d: first difference at %s" % (g, fmt, w, h, np.argwhere(got != want)[:3])
            if j != 1:
                continue
            src_d = mem.alloc(buf)
            dst_d = mem.alloc(np.zeros(want.size, dtype=np.uint8))
            pkg.convert_clip(src_d, cpf(pkg, g), w, h, fmt, n=n, out=dst_d)
            assert np.array_equal(mem.read(dst_d, want.size).reshape(want.shape), want), "device %s fmt 0x%x" % (g, fmt)
            ncases += 1
    assert ncases >= 40


@pytest.mark.parametrize("layout,depth,msb,fmt", [(PF.PLANAR, 10, 0, A.SUBSAMP_420), (PF.SEMI_UV, 8, 0, A.SUBSAMP_420), (PF.SEMI_UV, 10, 1, A.SUBSAMP_420),
                                                  (PF.SEMI_VU, 8, 0, A.SUBSAMP_420), (PF.YUYV, 8, 0, A.SUBSAMP_422), (PF.UYVY, 8, 0, A.SUBSAMP_422),
                                                  (PF.SEMI_UV, 16, 0, A.SUBSAMP_422), (PF.PLANAR, 12, 1, A.SUBSAMP_444)])
def test_1080p(pkg, layout, depth, msb, fmt):
    w, h = 1920, 1080
    f = PF.pf(layout, depth, msb)
    for g in (f, padded(f, w, h, fmt, pad=(128, 64, 64), stride_pad=4096)):
        buf, want = source(g, w, h, fmt, 2, depth * 10 + layout)
        assert np.array_equal(pkg.convert_clip(buf, cpf(pkg, g), w, h, fmt), want)


@pytest.mark.parametrize("w,h,soff,doff", [(352, 288, 4096, 4096), (250, 130, 4096 + 3, 4096 + 5), (36, 20, 4096 + 16, 4096 + 1)])
def test_canary(pkg, mem, w, h, soff, doff):
    """source and destination exactly n frames long inside larger allocations of a known pattern: the surroundings stay as they were
    (the surroundings are the test's own memory), the result is right at any buffer alignment"""
    n = 2
    for i, (f, fmt) in enumerate(valid_cases()):
        if f["depth"] not in (8, 10):
            continue
        g = padded(f, w, h, fmt, pad=(16, 32, 16), stride_pad=64) if i % 2 else f
        buf, want = source(g, w, h, fmt, n, 77 + i)
        assert buf.size == n * PF.frame_bytes(g, w, h, fmt)
        big_s = np.full(soff + buf.size + 4096, 0xC3, dtype=np.uint8)
        big_s[soff:soff + buf.size] = buf
        big_d = np.full(doff + want.size + 4096, 0x3C, dtype=np.uint8)
        ps, pd = mem.alloc(big_s), mem.alloc(big_d)
        pkg.convert_clip(C.c_void_p(ps.value + soff), cpf(pkg, g), w, h, fmt, n=n, out=C.c_void_p(pd.value + doff))
        after_d, after_s = mem.read(pd, big_d.size), mem.read(ps, big_s.size)
        assert np.array_equal(after_s, big_s), "the source allocation changed (%s)" % (g,)
        assert (after_d[:doff] == 0x3C).all() and (after_d[doff + want.size:] == 0x3C).all(), "written outside the destination (%s)" % (g,)
        assert np.array_equal(after_d[doff:doff + want.size], want.reshape(-1)), (g, fmt)


# ---- batches -------------------------------------------------------------------------------------------------------------------
BATCH_FORMATS = {"nv12": (PF.pf(PF.SEMI_UV), A.SUBSAMP_420), "p010": (PF.pf(PF.SEMI_UV, 10, 1), A.SUBSAMP_420),
                 "yuyv": (PF.pf(PF.YUYV), A.SUBSAMP_422), "yuv420p10": (PF.pf(PF.PLANAR, 10, 0), A.SUBSAMP_420)}


def raw_of(clip, f, w, h, fmt, seed=5, pad=True):
    """a planar 8-bit clip [n, frame_bytes] laid out in format f (padded) with its low bits random -> (raw [n, raw frame bytes], format)"""
    rng = np.random.default_rng(seed)
    g = padded(f, w, h, fmt, pad=(32, 16, 16), stride_pad=128) if pad else f
    vals = clip.astype(np.uint32)
    if f["depth"] > 8:
        s = f["depth"] - 8                              # values that round to the clip's: x * 2^s + [-2^(s-1), 2^(s-1))
        vals = np.clip((vals << s).astype(np.int64) + rng.integers(-(1 << (s - 1)), 1 << (s - 1), vals.shape), 0, (1 << f["depth"]) - 1).astype(np.uint32)
    raw = PF.pack(vals, g, w, h, fmt, rng).reshape(clip.shape[0], -1)
    return raw, g


def run_batch(pkg, calls, cfg, S, F, g=None, mode="host", pipelined=True, opener=None):
    """calls: list of [S, F, bytes] arrays -> streams (bytes per output stream)"""
    b = opener() if opener else pkg.Batch(cfg, S, F)
    try:
        if g is not None:
            b.set_source_format(cpf(pkg, g))
        dev = mode in ("device", "held")
        junk = np.full(calls[0].size, 0xA5, dtype=np.uint8)
        ins = [b.upload(c) for c in calls] if dev else calls
        got = [b""] * b.nstreams

        def submit(c):
            b.submit(c, on_device=dev, held=mode == "held")
            if mode == "device":                         # a plain device clip is the caller's again when submit returns
                assert b.L.dsvg_dev_upload(b.ctx, c, junk.ctypes.data, junk.nbytes) == 0

        def take(part):
            got[:] = [x + bytes(p) for x, p in zip(got, part)]

        if pipelined:
            submit(ins[0])
            for k in range(1, len(ins)):
                submit(ins[k])                           # two batches in flight
                take(b.collect())
            take(b.collect())
        else:
            for c in ins:
                take(b.encode(c, on_device=dev))
    finally:
        b.close()
    return got


@pytest.mark.parametrize("name", sorted(BATCH_FORMATS))
@pytest.mark.parametrize("rate", ["crf", "abr"])
def test_batch_with_source_format(pkg, orc, name, rate):
    f, fmt = BATCH_FORMATS[name]
    w, h, S, F, n = 176, 144, 2, 4, 12
    base = CRF if rate == "crf" else ABR
    clips = [A.gen_clip(w, h, fmt, 0x91F + s, n, style=(0, 3)[s]) for s in range(S)]
    raws = [raw_of(c, f, w, h, fmt, seed=s) for s, c in enumerate(clips)]
    g = raws[0][1]
    conv = [PF.convert(r.reshape(-1), g, w, h, fmt, n) for r, _ in raws]
    for c, k in zip(clips, conv):
        assert np.array_equal(c, k)                      # (the raw clip's low bits round away)
    want = [A.orc_encode(c, A.orc_cfg(w, h, fmt, **dict(base, qp=80)), eos=False)[0] for c in conv]
    cfg = pkg.make_encoder_cfg(w, h, fmt, **dict(base, qp=80))
    raw_calls = [np.ascontiguousarray(np.stack([r[k * F:(k + 1) * F] for r, _ in raws])) for k in range(n // F)]
    planar_calls = [np.ascontiguousarray(np.stack([c[k * F:(k + 1) * F] for c in conv])) for k in range(n // F)]
    plain = run_batch(pkg, planar_calls, cfg, S, F)
    assert plain == want
    for mode, pipelined in [("host", True), ("device", True), ("held", True), ("host", False), ("device", False)]:
        got = run_batch(pkg, raw_calls, cfg, S, F, g=g, mode=mode, pipelined=pipelined)
        assert got == plain, "%s %s %s pipelined=%s: not the bytes of the converted planar clip" % (name, rate, mode, pipelined)
        assert got == want


def test_quality_ladder_and_chain_mode(pkg, orc):
    w, h, fmt, F, n = 176, 144, A.SUBSAMP_420, 4, 8
    f = PF.pf(PF.SEMI_UV, 10, 1)
    clips = [A.gen_clip(w, h, fmt, 0x1AD + s, n, style=s + 1) for s in range(2)]
    raws = [raw_of(c, f, w, h, fmt, seed=9 + s) for s, c in enumerate(clips)]
    g = raws[0][1]
    qps = (60, 90)
    rungs = [pkg.make_encoder_cfg(w, h, fmt, **dict(CRF, qp=q)) for q in qps]
    calls = [np.ascontiguousarray(np.stack([r[k * F:(k + 1) * F] for r, _ in raws])) for k in range(n // F)]
    for mode in ("host", "held"):
        got = run_batch(pkg, calls, None, 2, F, g=g, mode=mode, opener=lambda: pkg.Ladder(rungs, 2, F))
        for s in range(2):
            for r, q in enumerate(qps):
                assert got[s * 2 + r] == A.orc_encode(clips[s], A.orc_cfg(w, h, fmt, **dict(CRF, qp=q)), eos=False)[0], (mode, s, r)
    # chain mode: one stream, consecutive frames, NV12
    f = PF.pf(PF.SEMI_UV)
    clip = A.gen_clip(w, h, fmt, 0xC4A1, 16, style=3)
    raw, g = raw_of(clip, f, w, h, fmt)
    cfg = pkg.make_encoder_cfg(w, h, fmt, **dict(CRF, qp=75, gop=6))
    calls = [np.ascontiguousarray(raw[k * 8:(k + 1) * 8][None]) for k in range(2)]
    want = A.orc_encode(clip, A.orc_cfg(w, h, fmt, **dict(CRF, qp=75, gop=6)), eos=False)[0]
    for mode in ("host", "device"):
        got = run_batch(pkg, calls, cfg, 1, 8, g=g, mode=mode, pipelined=False, opener=lambda: pkg.Batch(cfg, 1, 8, chains=2))
        assert got[0] == want, mode


def test_batch_error_contract_and_switching_back(pkg, orc):
    w, h, fmt, S, F = 176, 144, A.SUBSAMP_420, 1, 4
    L = pkg.lib()
    clip = A.gen_clip(w, h, fmt, 0xE44, 2 * F, style=1)
    raw, g = raw_of(clip, PF.pf(PF.SEMI_UV), w, h, fmt)
    cfg = pkg.make_encoder_cfg(w, h, fmt, **dict(CRF, qp=80))
    want = A.orc_encode(clip, A.orc_cfg(w, h, fmt, **dict(CRF, qp=80)), eos=False)[0]
    b = pkg.Batch(cfg, S, F)
    try:
        assert L.dsv1_batch_set_source_format(b.h, C.byref(cpf(pkg, PF.pf(PF.YUYV)))) == DSVG_ERR_ARG      # 4:2:0 stream
        assert L.dsv1_batch_set_source_format(b.h, C.byref(cpf(pkg, PF.pf(PF.SEMI_UV, pitch=(w - 1, 0, 0))))) == DSVG_ERR_ARG
        b.set_source_format(cpf(pkg, g))
        with pytest.raises(ValueError):
            b.submit(clip[:F][None])                     # the input-length check follows the format
        pin = b.pinned((S, F, raw.shape[1]))
        pin[...] = raw[:F][None]
        assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == DSVG_ERR_ARG
        b.submit(pin)
        assert L.dsv1_batch_set_source_format(b.h, None) == DSVG_ERR_ARG                  # a batch in flight
        assert L.dsv1_batch_set_source_format(b.h, C.byref(cpf(pkg, g))) == DSVG_ERR_ARG
        first = b.collect()[0]
        b.set_source_format(None)                        # back to packed planar: the second half of the stream from the planar clip
        second = b.encode(clip[F:][None])[0]
        assert first + second == want
        b.set_source_format(cpf(pkg, PF.pf()))           # planar / 8 / tight is the default too
        assert b.frame_bytes == A.frame_bytes(w, h, fmt)
    finally:
        b.close()


# ---- resolution ladders --------------------------------------------------------------------------------------------------------
def plane_sse(a, b, w, h, fmt):
    out = np.zeros(3, dtype=np.uint64)
    for p, (x, y) in enumerate(zip(RS.planes(a, w, h, fmt), RS.planes(b, w, h, fmt))):
        d = x.astype(np.int64) - y.astype(np.int64)
        out[p] = int((d * d).sum())
    return out


@pytest.mark.parametrize("name,mode", [("nv12", "host"), ("nv12", "device"), ("p010", "host"), ("p010", "held")])
def test_resolution_ladder_open_src(pkg, orc, name, mode):
    f, fmt = BATCH_FORMATS[name]
    w, h, S, F, n = 176, 144, 2, 4, 8
    geoms = [(w, h, [dict(qp=80)]), (128, 96, [dict(qp=60), dict(qp=90)]), (96, 72, [dict(qp=70)])]
    clips = [A.gen_clip(w, h, fmt, 0x5EC + s, n, style=(0, 3)[s]) for s in range(S)]
    raws = [raw_of(c, f, w, h, fmt, seed=20 + s) for s, c in enumerate(clips)]
    g = raws[0][1]
    conv = [PF.convert(r.reshape(-1), g, w, h, fmt, n) for r, _ in raws]
    want = []
    for clip in conv:
        for gw, gh, rates in geoms:
            sc = clip if (gw, gh) == (w, h) else Z.scale_clip(clip, w, h, fmt, gw, gh, Z.CUBIC)
            for rate in rates:
                data, recs = A.orc_encode(sc, A.orc_cfg(gw, gh, fmt, **dict(CRF, **rate)), want_recon=True, eos=False)
                q = [RS.src_quality(clip[t], r, w, h, gw, gh, fmt, Z.CUBIC) for t, r in enumerate(recs)]
                want.append((data, np.stack([plane_sse(sc[t], r, gw, gh, fmt) for t, r in enumerate(recs)]),
                             np.stack([SS.picture_fx(sc[t], r, gw, gh, fmt) for t, r in enumerate(recs)]),
                             np.stack([a for a, _ in q]), np.stack([x for _, x in q])))
    b = pkg.ResLadder(w, h, fmt, [(gw, gh, [pkg.make_encoder_cfg(gw, gh, fmt, **dict(CRF, **r)) for r in rates]) for gw, gh, rates in geoms],
                      S, F, Z.CUBIC, src_format=cpf(pkg, g))
    try:
        b.sse_enable()
        b.ssim_enable()
        b.src_quality_enable(filt=Z.CUBIC)
        calls = [np.ascontiguousarray(np.stack([r[k * F:(k + 1) * F] for r, _ in raws])) for k in range(n // F)]
        dev = mode != "host"
        junk = np.full(calls[0].size, 0x5A, dtype=np.uint8)
        ins = [b.upload(c) for c in calls] if dev else calls
        got, figs = [b""] * b.nstreams, [[], [], [], []]

        def submit(c):
            b.submit(c, on_device=dev, held=mode == "held")
            if mode == "device":
                assert b.L.dsvg_dev_upload(b.ctx, c, junk.ctypes.data, junk.nbytes) == 0

        def take(part):
            got[:] = [x + bytes(p) for x, p in zip(got, part)]
            for i, fn in enumerate((b.sse, b.ssim_fx, b.src_sse, b.src_ssim_fx)):
                figs[i].append(fn())

        submit(ins[0])
        submit(ins[1])
        take(b.collect())
        take(b.collect())
        up = b.uploads()
    finally:
        b.close()
    figs = [np.concatenate(x, axis=1) for x in figs]
    assert up == ((calls[0].nbytes * len(calls), len(calls)) if mode == "host" else (0, 0))
    assert calls[0].nbytes == S * F * PF.frame_bytes(g, w, h, fmt)
    for k, (data, sse, fx, xsse, xfx) in enumerate(want):
        assert got[k] == data, "output stream %d: packets differ from the oracle's" % k
        for i, e in enumerate((sse, fx, xsse, xfx)):
            assert np.array_equal(figs[i][k], e), "output stream %d: figure %d differs: %s vs %s" % (k, i, figs[i][k][:2], e[:2])
