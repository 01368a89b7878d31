"""RGB in and out on the GPU (include/dsv1_api.h, RGB; csrc/k_rgb.hip): dsv1_rgb_import_clip and dsv1_rgb_export_clip equal the numpy
statement tests/_rgb.py byte for byte -- every order, matrix, range, subsampling and upsampling mode, on the 16-byte path, the byte
path and mixed, host and device memory, guard bytes and padding as they were; batches, quality ladders, chain mode and resolution
ladders fed RGB write the oracle's streams of the numpy-converted clip; the batched decoder writes RGB frames of the oracle's
pictures, through the int32 second pass and a rebuilt context too."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import _pixfmt as PF
import _pixout as PO
import _resample as RS
import _rgb as RG
import _scale as Z
import blocksize_cases as BC
from test_gpu_pixfmt import CRF, DevMem, cpf, plane_sse, raw_of, run_batch
from test_gpu_pixout import streams_of
from test_gpu_decode_escape import _two_picture_stream, plane_payload, region_base, splice

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2
GUARD = 256
PAIRS = [(m, r) for m in RG.MATRICES for r in (0, 1)]


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return m


@pytest.fixture
def mem(pkg):
    m = DevMem(pkg)
    yield m
    m.close()


def crf(pkg, f):
    return pkg.RgbFormat(f["order"], f["matrix"], f["full"], f["upsample"], f["pitch"], f["frame_bytes"])


def padded(f, w, h, pad=(48, 16, 80), stride_pad=256):
    """pitches and a frame stride beyond the rows, multiples of 16 or not as `pad` says"""
    lay, _, _ = RG.layout(f, w, h)
    g = dict(f, pitch=tuple(lay[k][2] + pad[k] if k < len(lay) else 0 for k in range(3)))
    return dict(g, frame_bytes=RG.layout(g, w, h)[1] + stride_pad)


def streams_fast(f, w, h, sub):
    """(RGB, Y, chroma): does every row of the stream start 16-byte aligned (8 for halved chroma) in every frame, with buffers that
    start aligned -- the kernels' rule for the 16-byte path of each of their three streams (csrc/k_rgb.hip)"""
    lay, _, fb = RG.layout(f, w, h)
    cw, ch = A.chroma_dims(w, h, sub)
    pfb = A.frame_bytes(w, h, sub)
    al = 8 if A.hshift(sub) else 16
    return (all((fb | off | pitch) % 16 == 0 for off, pitch, _ in lay), (pfb | w) % 16 == 0,
            (pfb | (w * h) | (w * h + cw * ch) | cw) % al == 0)


# the geometries of tests/test_gpu_pixout.py, for its reasons: 352x288 every row on the 16-byte path; 250x130 none aligned; 36x20 and
# 48x18 tails; 35x19 odd -- both clamps of the halving and of the upsampling; 1x1
GEOMS = [(352, 288), (250, 130), (36, 20), (35, 19), (1, 1), (48, 18)]
PADS = [None, dict(pad=(48, 16, 80), stride_pad=256), dict(pad=(5, 3, 7), stride_pad=37)]


def cases():
    """every order with every subsampling; every (matrix, range), padding and upsampling mode with every order's neighbours: each
    value of each axis appears at every geometry, not the full cross product"""
    for k, sub in enumerate(RG.SUBSAMPS):
        for order in RG.ORDERS:
            m, r = PAIRS[(order + k) % 6]
            yield RG.rf(order, m, r, (order + k) % 2), sub, PADS[(order + 2 * k) % 3]


def test_case_list_has_every_value_of_every_axis():
    cs = list(cases())
    assert {(f["order"], s) for f, s, _ in cs} == {(o, s) for o in RG.ORDERS for s in RG.SUBSAMPS}
    assert {(f["matrix"], f["full"]) for f, _, _ in cs} == set(PAIRS)
    for s in RG.SUBSAMPS:
        assert {f["upsample"] for f, x, _ in cs if x == s} == {RG.REPLICATE, RG.LINEAR}
        assert len({id(p) for _, x, p in cs if x == s}) == 3
    for o in RG.ORDERS:
        assert {f["upsample"] for f, _, _ in cs if f["order"] == o} == {RG.REPLICATE, RG.LINEAR}
        assert len({id(p) for f, _, p in cs if f["order"] == o}) == 3


def test_geometry_list_reaches_the_vector_path_the_byte_path_and_mixed_streams():
    """from the geometry alone"""
    S420, S422, S444 = A.SUBSAMP_420, A.SUBSAMP_422, A.SUBSAMP_444
    for g in [(352, 288), (250, 130), (36, 20), (35, 19), (48, 18), (1, 1)]:
        assert g in GEOMS
    for order in RG.ORDERS:
        f = RG.rf(order)
        for sub in RG.SUBSAMPS:
            assert streams_fast(f, 352, 288, sub) == (True, True, True)
            assert streams_fast(padded(f, 352, 288, **PADS[1]), 352, 288, sub) == (True, True, True)
            assert streams_fast(f, 250, 130, sub) == (False, False, False)
            # mixed: RGB rows off the 16-byte path, the planar side on it
            assert streams_fast(padded(f, 352, 288, **PADS[2]), 352, 288, sub) == (False, True, True)
    # 48x18: aligned rows of three whole steps; 4:2:0 chroma rows of 24 = three 8-byte stores
    assert streams_fast(RG.rf(RG.RGB24), 48, 18, S420) == (True, True, True) and A.chroma_dims(48, 18, S420) == (24, 9)
    # 36x20: two whole steps and a tail of 4 pixels; padded to aligned RGB rows the RGB stream is on the 16-byte path, Y and chroma not
    assert 36 // 16 == 2 and 36 % 16 == 4
    assert streams_fast(padded(RG.rf(RG.BGRA), 36, 20, **PADS[1]), 36, 20, S420) == (True, False, False)
    assert streams_fast(RG.rf(RG.PLANAR_RGB), 36, 20, S444) == (False, False, False)
    # 35x19: odd chroma planes (the repeated last column / row; the upsampling's edge clamps and its dropped last row)
    assert A.chroma_dims(35, 19, S420) == (18, 10) and A.chroma_dims(35, 19, S422) == (18, 19)


def rgb_source(w, h, n, rng):
    """random components with the extremes and the pure primaries in every clip (full-range pure blue and red reach 256 before the
    clamp)"""
    R, G, B = (rng.integers(0, 256, (n, h, w), dtype=np.uint8) for _ in range(3))
    prim = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]
    for t in range(n):
        for i, (r, g, b) in enumerate(prim):
            y, x = (i * 7 + t) % h, (i * 5) % w
            if w * h >= 8 or i == (4 if t == 0 else 2):
                R[t, y, x], G[t, y, x], B[t, y, x] = r, g, b
    return R, G, B


@pytest.mark.parametrize("w,h", GEOMS)
def test_rgb_import_clip_equals_numpy(pkg, mem, w, h):
    """host and device memory; the source allocation and the 256 guard bytes around the destination stay as they were"""
    n = 3
    for i, (f0, sub, pad) in enumerate(cases()):
        rng = np.random.default_rng(9000 + i)
        f = f0 if pad is None else padded(f0, w, h, **pad)
        R, G, B = rgb_source(w, h, n, rng)
        buf = RG.pack(R, G, B, f, w, h, rng)
        want = RG.import_(buf, f, w, h, sub, n)
        what = "%s %s 0x%x %dx%d" % (RG.NAMES[f["order"]], f, sub, w, h)
        got = pkg.rgb_import_clip(buf, crf(pkg, f), w, h, sub)
        assert got.shape == want.shape
        assert np.array_equal(got, want), "host %s: first difference at %s" % (what, np.argwhere(got != want)[:3])
        # the last frame may end with its planes
        short = buf[:(n - 1) * RG.frame_bytes(f, w, h) + RG.layout(f, w, h)[1]]
        assert pkg.lib().dsv1_rgb_import_clip(0, short.ctypes.data, C.byref(crf(pkg, f)), w, h, sub, n, got.ctypes.data, 0) == 0
        assert np.array_equal(got, want), "host, short last frame, %s" % what
        before = rng.integers(0, 256, GUARD + want.size + GUARD, dtype=np.uint8)
        src_d, dst_d = mem.alloc(buf), mem.alloc(before)
        pkg.rgb_import_clip(src_d, crf(pkg, f), w, h, sub, n=n, out=C.c_void_p(dst_d.value + GUARD))
        after = mem.read(dst_d, before.size)
        exp = before.copy()
        exp[GUARD:GUARD + want.size] = want.reshape(-1)
        assert np.array_equal(after, exp), "device %s: first difference at %s" % (what, np.argwhere(after != exp)[:3].ravel())
        assert np.array_equal(mem.read(src_d, buf.size), buf), "the source changed (%s)" % what


@pytest.mark.parametrize("w,h", GEOMS)
def test_rgb_export_clip_equals_numpy(pkg, mem, w, h):
    """whole destination compared, 256 guard bytes before and after included: padding and surroundings are as they were"""
    n = 3
    for i, (f0, sub, pad) in enumerate(cases()):
        rng = np.random.default_rng(9500 + i)
        f = f0 if pad is None else padded(f0, w, h, **pad)
        x = rng.integers(0, 256, (n, A.frame_bytes(w, h, sub)), dtype=np.uint8)
        x[:, :2], x[:, -2:] = 255, 0
        fb = RG.frame_bytes(f, w, h)
        before = rng.integers(0, 256, GUARD + n * fb + GUARD, dtype=np.uint8)
        want = before.copy()
        RG.export(x, f, w, h, sub, n, into=want[GUARD:GUARD + n * fb])
        what = "%s %s 0x%x %dx%d" % (RG.NAMES[f["order"]], f, sub, w, h)
        got = before.copy()
        pkg.rgb_export_clip(x, w, h, sub, crf(pkg, f), out=got[GUARD:GUARD + n * fb])
        assert np.array_equal(got, want), "host %s: first difference at %s" % (what, np.argwhere(got != want)[:3].ravel())
        src_d, dst_d = mem.alloc(x), mem.alloc(before)
        pkg.rgb_export_clip(src_d, w, h, sub, crf(pkg, f), n=n, out=C.c_void_p(dst_d.value + GUARD))
        got = mem.read(dst_d, before.size)
        assert np.array_equal(got, want), "device %s: first difference at %s" % (what, np.argwhere(got != want)[:3].ravel())


@pytest.mark.parametrize("w,h", [(352, 288), (35, 19)])
def test_import_at_a_subsampling_is_export_clip_of_the_444_import_on_the_device(pkg, mem, w, h):
    n = 2
    rng = np.random.default_rng(w)
    for order, (m, r) in zip((RG.RGB24, RG.ARGB, RG.PLANAR_GBR), ((RG.BT601, 1), (RG.BT709, 0), (RG.BT2020, 1))):
        f = RG.rf(order, m, r)
        buf = RG.pack(*rgb_source(w, h, n, rng), f, w, h, rng)
        src_d = mem.alloc(buf)
        d444 = mem.alloc(np.zeros(n * A.frame_bytes(w, h, A.SUBSAMP_444), dtype=np.uint8))
        pkg.rgb_import_clip(src_d, crf(pkg, f), w, h, A.SUBSAMP_444, n=n, out=d444)
        for sub in RG.SUBSAMPS:
            nb = n * A.frame_bytes(w, h, sub)
            a, b = mem.alloc(np.zeros(nb, dtype=np.uint8)), mem.alloc(np.zeros(nb, dtype=np.uint8))
            pkg.rgb_import_clip(src_d, crf(pkg, f), w, h, sub, n=n, out=a)
            pkg.export_clip(d444, w, h, A.SUBSAMP_444, cpf(pkg, PF.pf()), sub, n=n, out=b)
            assert np.array_equal(mem.read(a, nb), mem.read(b, nb)), (RG.NAMES[order], sub)


# ---- encoders --------------------------------------------------------------------------------------------------------------------
def rgb_clip(w, h, n, seed, style):
    """moving pictures as R, G, B [n, h, w]: the planes of a generated 4:4:4 clip"""
    c = A.gen_clip(w, h, A.SUBSAMP_444, seed, n, style=style).reshape(n, 3, h, w)
    return c[:, 2], c[:, 0], c[:, 1]


def raw_rgb(w, h, n, seed, style, f):
    return RG.pack(*rgb_clip(w, h, n, seed, style), f, w, h, np.random.default_rng(seed)).reshape(n, -1)


SOURCES = {"rgb24-420": (RG.rf(RG.RGB24, RG.BT709, 0), A.SUBSAMP_420, None, 176, 144),
           "bgra-422-padded": (RG.rf(RG.BGRA, RG.BT601, 1), A.SUBSAMP_422, dict(pad=(32, 0, 0), stride_pad=128), 176, 144),
           "gbrp-444": (RG.rf(RG.PLANAR_GBR, RG.BT2020, 0), A.SUBSAMP_444, dict(pad=(5, 3, 7), stride_pad=37), 64, 64)}


def opener_of(pkg, make, f):
    def go():
        b = make()
        b.set_source_rgb(crf(pkg, f))
        return b
    return go


@pytest.mark.parametrize("name", sorted(SOURCES))
def test_batch_with_rgb_source(pkg, orc, name):
    f, fmt, pad, w, h = SOURCES[name]
    S, F, n = 2, 4, 8
    if pad:
        f = padded(f, w, h, **pad)
    raws = [raw_rgb(w, h, n, 0x26B + s, (0, 3)[s], f) for s in range(S)]
    conv = [RG.import_(r.reshape(-1), f, w, h, fmt, n) for r in raws]
    want = [A.orc_encode(c, A.orc_cfg(w, h, fmt, **dict(CRF, qp=80)), eos=False)[0] for c in conv]
    cfg = pkg.make_encoder_cfg(w, h, fmt, **dict(CRF, qp=80))
    raw_calls = [np.ascontiguousarray(np.stack([r[k * F:(k + 1) * F] for r in raws])) for k in range(n // F)]
    planar_calls = [np.ascontiguousarray(np.stack([c[k * F:(k + 1) * F] for c in conv])) for k in range(n // F)]
    assert raw_calls[0].nbytes == S * F * RG.frame_bytes(f, w, h)
    assert run_batch(pkg, planar_calls, cfg, S, F) == want
    for mode, pipelined in [("host", True), ("device", True), ("held", True), ("host", False), ("device", False)]:
        got = run_batch(pkg, raw_calls, cfg, S, F, mode=mode, pipelined=pipelined, opener=opener_of(pkg, lambda: pkg.Batch(cfg, S, F), f))
        assert got == want, "%s %s pipelined=%s: not the oracle's bytes of the numpy-converted clip" % (name, mode, pipelined)


def test_quality_ladder_and_chain_mode_with_rgb_source(pkg, orc):
    w, h, fmt, F, n = 176, 144, A.SUBSAMP_420, 4, 8
    f = padded(RG.rf(RG.ABGR, RG.BT601, 0), w, h, pad=(16, 0, 0), stride_pad=64)
    raws = [raw_rgb(w, h, n, 0x1AD + s, s + 1, f) for s in range(2)]
    conv = [RG.import_(r.reshape(-1), f, w, h, fmt, n) for r in raws]
    qps = (60, 90)
    rungs = [pkg.make_encoder_cfg(w, h, fmt, **dict(CRF, qp=q)) for q in qps]
    calls = [np.ascontiguousarray(np.stack([r[k * F:(k + 1) * F] for r in raws])) for k in range(n // F)]
    want = {(s, r): A.orc_encode(conv[s], A.orc_cfg(w, h, fmt, **dict(CRF, qp=q)), eos=False)[0] for s in range(2) for r, q in enumerate(qps)}
    for mode in ("host", "device", "held"):
        got = run_batch(pkg, calls, None, 2, F, mode=mode, opener=opener_of(pkg, lambda: pkg.Ladder(rungs, 2, F), f))
        for (s, r), x in want.items():
            assert got[s * 2 + r] == x, (mode, s, r)
    # chain mode: one stream, consecutive frames, planar RGB
    f = RG.rf(RG.PLANAR_RGB, RG.BT709, 1)
    raw = raw_rgb(w, h, 16, 0xC4A1, 3, f)
    conv = RG.import_(raw.reshape(-1), f, w, h, fmt, 16)
    cfg = pkg.make_encoder_cfg(w, h, fmt, **dict(CRF, qp=75, gop=6))
    calls = [np.ascontiguousarray(raw[k * 8:(k + 1) * 8][None]) for k in range(2)]
    want = A.orc_encode(conv, A.orc_cfg(w, h, fmt, **dict(CRF, qp=75, gop=6)), eos=False)[0]
    for mode in ("host", "device", "held"):
        got = run_batch(pkg, calls, cfg, 1, 8, mode=mode, pipelined=False, opener=opener_of(pkg, lambda: pkg.Batch(cfg, 1, 8, chains=2), f))
        assert got[0] == want, mode


@pytest.mark.parametrize("mode", ["host", "device", "held"])
def test_resolution_ladder_open_rgb(pkg, orc, mode):
    w, h, fmt, S, F, n = 352, 288, A.SUBSAMP_420, 2, 2, 4
    f = padded(RG.rf(RG.BGR24, RG.BT709, 0), w, h, pad=(16, 0, 0), stride_pad=256)
    geoms = [(w, h, [dict(qp=80)]), (176, 144, [dict(qp=60), dict(qp=90)])]
    raws = [raw_rgb(w, h, n, 0x5EC + s, (0, 3)[s], f) for s in range(S)]
    conv = [RG.import_(r.reshape(-1), f, w, h, fmt, n) for r in raws]
    want = []
    for clip in conv:
        for gw, gh, rates in geoms:
            sc = clip if (gw, gh) == (w, h) else Z.scale_clip(clip, w, h, fmt, gw, gh, Z.CUBIC)
            for rate in rates:
                data, recs = A.orc_encode(sc, A.orc_cfg(gw, gh, fmt, **dict(CRF, **rate)), want_recon=True, eos=False)
                want.append((data, np.stack([plane_sse(sc[t], r, gw, gh, fmt) for t, r in enumerate(recs)]),
                             np.stack([RS.src_quality(clip[t], r, w, h, gw, gh, fmt, Z.CUBIC)[0] for t, r in enumerate(recs)])))
    b = pkg.ResLadder(w, h, fmt, [(gw, gh, [pkg.make_encoder_cfg(gw, gh, fmt, **dict(CRF, **r)) for r in rates]) for gw, gh, rates in geoms],
                      S, F, Z.CUBIC, src_rgb=crf(pkg, f))
    try:
        assert b.frame_bytes == RG.frame_bytes(f, w, h)
        b.sse_enable()
        b.src_quality_enable(filt=Z.CUBIC)
        calls = [np.ascontiguousarray(np.stack([r[k * F:(k + 1) * F] for r in raws])) for k in range(n // F)]
        dev = mode != "host"
        junk = np.full(calls[0].size, 0x5A, dtype=np.uint8)
        ins = [b.upload(c) for c in calls] if dev else calls
        got, figs = [b""] * b.nstreams, [[], []]

        def submit(c):
            b.submit(c, on_device=dev, held=mode == "held")
            if mode == "device":                         # a plain device clip is the caller's again when submit returns
                assert b.L.dsvg_dev_upload(b.ctx, c, junk.ctypes.data, junk.nbytes) == 0

        def take(part):
            got[:] = [x + bytes(p) for x, p in zip(got, part)]
            for i, fn in enumerate((b.sse, b.src_sse)):
                figs[i].append(fn())

        submit(ins[0])
        submit(ins[1])
        take(b.collect())
        take(b.collect())
        up = b.uploads()
    finally:
        b.close()
    figs = [np.concatenate(x, axis=1) for x in figs]
    assert calls[0].nbytes == S * F * RG.frame_bytes(f, w, h)
    assert up == ((calls[0].nbytes * len(calls), len(calls)) if mode == "host" else (0, 0))          # the RGB bytes
    for k, (data, sse, xsse) in enumerate(want):
        assert got[k] == data, "output stream %d: packets differ from the oracle's" % k
        assert np.array_equal(figs[0][k], sse), "output stream %d: sse" % k
        assert np.array_equal(figs[1][k], xsse), "output stream %d: source-resolution sse is not against the converted clip" % k


# ---- batched decoder -------------------------------------------------------------------------------------------------------------
def run_decoder_rgb(pkg, packets, want, w, h, fmt, f, on_device, pitch_extra=0, seed=3):
    """decode the streams call by call with RGB output; after every call the WHOLE output buffer is compared with a host copy into
    which _rgb.export wrote the frames of the streams that had a picture -- the other streams' frames, every padding byte and the
    bytes between a frame and out_pitch keep the sentinel"""
    S = len(packets)
    d = pkg.DecBatch(w, h, fmt, S)
    try:
        d.set_output_rgb(crf(pkg, f))
        fb = RG.frame_bytes(f, w, h)
        assert d.frame_bytes == fb == pkg.lib().dsv1_decbatch_out_frame_bytes(d.h)
        d.frame_bytes = pitch = fb + pitch_extra          # (decode() passes it as out_pitch and sizes the buffers by it)
        eos = bytes(packets[0][-1])
        count = [0] * S
        expect = np.random.default_rng(seed).integers(0, 256, S * pitch, dtype=np.uint8)     # the sentinel
        if on_device:
            dev = d.dev_alloc()
            assert d.L.dsvg_dev_upload(d.ctx, dev, expect.ctypes.data, expect.nbytes) == 0
        else:
            host = expect.copy().reshape(S, pitch)
        for k in range(max(len(p) for p in packets)):
            pk = [packets[s][k] if k < len(packets[s]) else eos for s in range(S)]
            if on_device:
                _, status, fnum = d.decode(pk, out=dev, on_device=True)
                got = d.download(dev).reshape(-1)
            else:
                _, status, fnum = d.decode(pk, out=host)
                got = host.reshape(-1)
            for s in range(S):
                if k < len(packets[s]) and packets[s][k][5] & 4:
                    assert status[s] == 0 and fnum[s] == count[s], (s, k, status[s], fnum[s])
                    RG.export(want[s][count[s]][None], f, w, h, fmt, 1, into=expect[s * pitch:s * pitch + fb])
                    count[s] += 1
                else:
                    assert status[s] in (2, 3)
            assert np.array_equal(got, expect), "call %d: first difference at byte %s (pitch %d)" % (k, np.argwhere(got != expect)[:3].ravel(), pitch)
        return count
    finally:
        d.close()


OUTPUTS = {
    "420-rgb24-linear":        (352, 288, A.SUBSAMP_420, RG.rf(RG.RGB24, RG.BT709, 0, RG.LINEAR), None, 0),
    "420-abgr-replicate":      (352, 288, A.SUBSAMP_420, RG.rf(RG.ABGR, RG.BT601, 1, RG.REPLICATE), None, 4096),
    "444-bgra-padded":         (320, 240, A.SUBSAMP_444, RG.rf(RG.BGRA, RG.BT2020, 0, RG.LINEAR), dict(pad=(48, 0, 0), stride_pad=256), 0),
    "422-planar-rgb-linear":   (360, 200, A.SUBSAMP_422, RG.rf(RG.PLANAR_RGB, RG.BT601, 0, RG.LINEAR), dict(pad=(5, 3, 7), stride_pad=37), 100),
    "422-bgr24-replicate":     (360, 200, A.SUBSAMP_422, RG.rf(RG.BGR24, RG.BT709, 1, RG.REPLICATE), None, 0),
}


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("name", sorted(OUTPUTS))
def test_batched_decoder_writes_rgb(pkg, orc, name, on_device):
    """streams of different lengths: a stream without a picture in a call keeps its bytes"""
    w, h, fmt, f, pad, extra = OUTPUTS[name]
    if pad:
        f = padded(f, w, h, **pad)
    _, packets, want = streams_of(w, h, fmt)
    assert run_decoder_rgb(pkg, packets, want, w, h, fmt, f, on_device, pitch_extra=extra) == [len(x) for x in want]


def test_escape_redo_keeps_rgb(pkg, orc):
    """a P picture with a symbol beyond int16 (tests/test_gpu_decode_escape.py) is decoded again from int32 coefficients after its
    RGB frame was already written on the device: the second pass writes RGB again, not a stale or a planar frame"""
    w, h, fmt, S = 352, 288, A.SUBSAMP_444, 4
    pk, ip = _two_picture_stream(w, h, fmt, 0xE5CA9E)
    b2, sw2 = region_base(w, h, 2, 1)
    b1, sw1 = region_base(w, h, 1, 2)
    entries = sorted([(5, 3), (b1 + 4 * sw1 + 9, -2), (b2 + 10 * sw2 + 10, 40000), (b2 + 30 * sw2 + 77, 1)])
    pk[ip] = splice(pk[ip], {0: plane_payload(7, entries)})
    want = A.orc_decode(b"".join(pk), w, h, fmt)
    assert len(want) == 2
    L = pkg.lib()
    L.dsvg_ctx_decoder_redone.restype = C.c_long
    L.dsvg_ctx_decoder_redone.argtypes = [C.c_void_p]
    f = RG.rf(RG.RGBA, RG.BT709, 0)
    d = pkg.DecBatch(w, h, fmt, S)
    try:
        d.set_output_rgb(crf(pkg, f))
        k = 0
        for p in pk:
            before = L.dsvg_ctx_decoder_redone(d.ctx)
            _, status, fnum = d.decode([p] * S, on_device=True)
            if status[0] == 0 and (p[5] & 4):
                frames = d.download()                    # (synchronises: the flags are settled here)
                exp = RG.export(want[k][None], f, w, h, fmt, 1)
                for s in range(S):
                    assert np.array_equal(frames[s], exp), "picture %d stream %d: first difference at %s" % (k, s, np.argwhere(frames[s] != exp)[:3].ravel())
                assert L.dsvg_ctx_decoder_redone(d.ctx) - before == (1 if k == 1 else 0)
                k += 1
        assert k == 2
    finally:
        d.close()


def test_the_setting_survives_a_context_rebuild(pkg, orc):
    """streams whose block size is not the rule's (tests/blocksize_cases.py): the batch builds a new context at their first picture,
    after the format was set"""
    w, h, fmt, n, stream = BC.make_stream(0)
    assert BC.CASES[0][6][0] == "32x24" and tuple(A.block_dims(w, h)[:2]) != (32, 24)
    want = A.orc_decode(stream, w, h, fmt)
    f = RG.rf(RG.BGR24, RG.BT601, 0, RG.LINEAR)
    d = pkg.DecBatch(w, h, fmt, 2)
    try:
        d.set_output_rgb(crf(pkg, f))
        t = 0
        for p in A.split_packets(stream):
            out, status, fnum = d.decode([p] * 2)
            if p[5] & 4:
                assert list(status) == [0, 0]
                exp = RG.export(want[t][None], f, w, h, fmt, 1)
                assert np.array_equal(out[0], exp) and np.array_equal(out[1], exp), t
                t += 1
        assert t == n
    finally:
        d.close()


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_411_is_refused_both_ways(pkg):
    L = pkg.lib()
    w, h = 64, 64
    good = crf(pkg, RG.rf())
    buf = np.zeros(3 * w * h, dtype=np.uint8)
    out = np.zeros(3 * w * h, dtype=np.uint8)
    assert L.dsv1_rgb_import_clip(0, buf.ctypes.data, C.byref(good), w, h, A.SUBSAMP_411, 1, out.ctypes.data, 0) == DSVG_ERR_ARG
    assert L.dsv1_rgb_export_clip(0, buf.ctypes.data, w, h, A.SUBSAMP_411, 1, out.ctypes.data, C.byref(good), 0) == DSVG_ERR_ARG
    assert not out.any()
    b = pkg.Batch(pkg.make_encoder_cfg(w, h, A.SUBSAMP_411), 1, 1)
    d = pkg.DecBatch(w, h, A.SUBSAMP_411, 1)
    try:
        assert L.dsv1_batch_set_source_rgb(b.h, C.byref(good)) == DSVG_ERR_ARG
        assert L.dsv1_decbatch_set_output_rgb(d.h, C.byref(good)) == DSVG_ERR_ARG
        with pytest.raises(ValueError):
            d.set_output_rgb(good)
        assert d.frame_bytes == A.frame_bytes(w, h, A.SUBSAMP_411)
    finally:
        b.close()
        d.close()


def test_batch_error_contract_and_the_setters_replacing_each_other(pkg, orc):
    w, h, fmt, S, F = 176, 144, A.SUBSAMP_420, 1, 4
    L = pkg.lib()
    f = RG.rf(RG.BGRA, RG.BT709, 0)
    raw = raw_rgb(w, h, 3 * F, 0xE44, 1, f)
    clip = RG.import_(raw.reshape(-1), f, w, h, fmt, 3 * F)
    nv12_raw, nv12 = raw_of(clip, PF.pf(PF.SEMI_UV), w, h, fmt, pad=False)
    cfg = pkg.make_encoder_cfg(w, h, fmt, **dict(CRF, qp=80))
    want = A.orc_encode(clip, A.orc_cfg(w, h, fmt, **dict(CRF, qp=80)), eos=False)[0]
    b = pkg.Batch(cfg, S, F)
    try:
        planar_fb = b.frame_bytes
        assert L.dsv1_batch_set_source_rgb(b.h, C.byref(crf(pkg, dict(f, matrix=5)))) == DSVG_ERR_ARG
        assert b.frame_bytes == planar_fb
        b.set_source_format(cpf(pkg, nv12))              # replaced by the RGB setter ...
        b.set_source_rgb(crf(pkg, f))
        assert b.frame_bytes == 4 * w * h
        # an invalid format leaves the setting in force
        assert L.dsv1_batch_set_source_rgb(b.h, C.byref(crf(pkg, dict(f, pitch=(4 * w - 1, 0, 0))))) == DSVG_ERR_ARG
        with pytest.raises(ValueError):
            b.submit(clip[:F][None])                     # the input-length check follows the format
        pin = b.pinned((S, F, raw.shape[1]))
        pin[...] = raw[:F][None]
        assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == DSVG_ERR_ARG
        b.submit(pin)
        assert L.dsv1_batch_set_source_rgb(b.h, None) == DSVG_ERR_ARG                     # a batch in flight
        assert L.dsv1_batch_set_source_rgb(b.h, C.byref(crf(pkg, f))) == DSVG_ERR_ARG
        assert L.dsv1_batch_set_source_format(b.h, C.byref(cpf(pkg, nv12))) == DSVG_ERR_ARG
        first = b.collect()[0]
        b.set_source_format(cpf(pkg, nv12))              # ... and the other way round: NV12 of the same converted clip
        assert b.frame_bytes == PF.frame_bytes(nv12, w, h, fmt)
        second = b.encode(nv12_raw[F:2 * F][None])[0]
        b.set_source_rgb(crf(pkg, f))
        b.set_source_rgb(None)                           # back to packed planar: the last third from the planar clip
        assert b.frame_bytes == planar_fb
        third = b.encode(clip[2 * F:][None])[0]
        assert first + second + third == want
    finally:
        b.close()


def test_decoder_setters_replace_each_other_and_refusals(pkg, orc):
    w, h, fmt = 352, 288, A.SUBSAMP_420
    L = pkg.lib()
    _, packets, want = streams_of(w, h, fmt)
    f = RG.rf(RG.RGB24, RG.BT709, 0, RG.LINEAR)
    fb = 3 * w * h
    d = pkg.DecBatch(w, h, fmt, 1)
    try:
        d.set_output_format(cpf(pkg, PF.pf(PF.SEMI_UV, 10, 1)))
        d.set_output_rgb(crf(pkg, f))
        assert d.frame_bytes == fb == L.dsv1_decbatch_out_frame_bytes(d.h)
        for bad in (dict(f, order=9), dict(f, upsample=3), dict(f, pitch=(3 * w - 1, 0, 0)), dict(f, frame_bytes=fb - 1), dict(f, full=2)):
            assert L.dsv1_decbatch_set_output_rgb(d.h, C.byref(crf(pkg, bad))) == DSVG_ERR_ARG, bad
            with pytest.raises(ValueError):
                d.set_output_rgb(crf(pkg, bad))
            assert d.frame_bytes == fb == L.dsv1_decbatch_out_frame_bytes(d.h)
        out = np.full((1, fb), 0x5A, dtype=np.uint8)
        status, fnum = (C.c_int * 1)(), (C.c_uint32 * 1)()
        t = 0
        plan = ["rgb", "rgb", "nv12", "planar"]
        for p in packets[0][:8]:
            if not p[5] & 4 or t >= len(plan):
                continue
            buf = (pkg.Buf * 1)()
            keep = np.frombuffer(bytes(p) + b"\0" * 16, dtype=np.uint8).copy()
            buf[0].data, buf[0].len = keep.ctypes.data_as(C.POINTER(C.c_uint8)), len(p)
            if plan[t] == "nv12":
                d.set_output_format(cpf(pkg, PF.pf(PF.SEMI_UV)))          # replaces the RGB setting
            elif plan[t] == "planar":
                d.set_output_rgb(crf(pkg, f))
                d.set_output_rgb(None)                                    # NULL switches back
            nb = d.frame_bytes
            if plan[t] == "rgb":                         # an output pitch below the frame: refused, nothing written
                held = out.copy()
                assert L.dsv1_decbatch_decode(d.h, buf, out.ctypes.data, fb - 1, 0, status, fnum) == DSVG_ERR_ARG
                assert np.array_equal(out, held)
            assert L.dsv1_decbatch_decode(d.h, buf, out.ctypes.data, 0, 0, status, fnum) == 0 and status[0] == 0
            exp = {"rgb": lambda: RG.export(want[0][t][None], f, w, h, fmt, 1),
                   "nv12": lambda: PO.export(want[0][t][None], PF.pf(PF.SEMI_UV), w, h, fmt, fmt, 1),
                   "planar": lambda: want[0][t].reshape(-1)}[plan[t]]()
            assert nb == exp.size and np.array_equal(out[0, :nb], exp), (t, plan[t])
            t += 1
        assert t == len(plan)
    finally:
        d.close()
    assert L.dsv1_decbatch_set_output_rgb(None, None) == DSVG_ERR_ARG
