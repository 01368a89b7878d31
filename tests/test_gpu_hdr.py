"""HDR sources on the GPU (include/dsv1_api.h, HDR sources; csrc/k_hdr.hip): dsv1_hdr_import_clip equals the numpy statement
tests/_hdr.py byte for byte -- every layout, depth, subsampling pair and upsampling mode, built and random tables, on the 16-byte
path and the byte path, host and device memory, guard bytes and padding as they were; batches, quality ladders, chain mode and
resolution ladders fed HDR clips write the streams of the same session fed the converted clip."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import _hdr as HD
import _pixfmt as PF
import _rgb as RG
from test_gpu_pixfmt import CRF, DevMem, cpf, run_batch

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2
GUARD = 256
S420, S422, S444 = A.SUBSAMP_420, A.SUBSAMP_422, A.SUBSAMP_444


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return m


@pytest.fixture(scope="module")
def mem(pkg):
    m = DevMem(pkg)
    yield m
    m.close()


def chd(pkg, h):
    return pkg.Hdr(h["transfer"], h["matrix"], h["full"], h["gamut"], h["curve"], h["peak"], h["white"], h["out_matrix"], h["out_full"])


@pytest.fixture(scope="module")
def tables(pkg):
    """[(name, tables as a dict, HdrTables)]: the library's tables of every curve and transfer, and tables of random entries inside the
    valid bounds -- built once, shared, never changed"""
    out = []
    for transfer in (HD.PQ, HD.HLG):
        for curve in HD.CURVES:
            t = pkg.hdr_build(chd(pkg, HD.hd(transfer, curve=curve, full=curve == HD.REINHARD, out_full=curve == HD.CLIP)))
            out.append(("built-%d-%d" % (transfer, curve), t.as_dict(), t))
    rng = np.random.default_rng(0x4D2)
    for k in range(2):
        d = HD.random_tables(rng)
        out.append(("random-%d" % k, d, pkg.HdrTables.from_dict(d)))
    return out


# planar 10 lsb, 12 (msb), 16; P010 and its VU twin; P210; planar 4:4:4 10-bit is planar 10 lsb at the 4:4:4 pairs
FORMATS = {"p10": PF.pf(PF.PLANAR, 10, 0), "p12": PF.pf(PF.PLANAR, 12, 1), "p16": PF.pf(PF.PLANAR, 16, 0), "P010": PF.pf(PF.SEMI_UV, 10, 1),
           "P010vu": PF.pf(PF.SEMI_VU, 10, 1), "P210": PF.pf(PF.SEMI_UV, 10, 1), "P212lsb": PF.pf(PF.SEMI_VU, 12, 0)}


def combos():
    """(name, format, src_subsamp, subsamp): every planar depth at every pair, the semi-planar layouts at the pairs they exist at"""
    for name in ("p10", "p12", "p16"):
        for a, b in HD.PAIRS:
            yield name, FORMATS[name], a, b
    for name, pairs in (("P010", [(S420, S420)]), ("P010vu", [(S420, S420)]), ("P210", [(S422, S422), (S422, S420)]), ("P212lsb", [(S422, S420), (S422, S422)])):
        for a, b in pairs:
            yield name, FORMATS[name], a, b


# (w, h, extra bytes of every pitch, n, extra bytes of the frame stride)
GEOMS = [(1, 1, 0, 1, 0), (2, 2, 0, 3, 64), (15, 3, 0, 1, 0), (17, 5, 0, 3, 64), (33, 2, 0, 1, 0), (64, 16, 0, 1, 0), (160, 32, 0, 3, 64),
         (48, 18, 3, 3, 64), (48, 18, 16, 1, 0)]


def fmt_for(f, w, h, sub, pitch_extra, stride_extra):
    lay, _, _ = PF.plane_layout(f, w, h, sub)
    g = dict(f, pitch=tuple(lay[k][2] + pitch_extra if k < len(lay) and pitch_extra else 0 for k in range(3)))
    return dict(g, frame_bytes=PF.plane_layout(g, w, h, sub)[1] + stride_extra if stride_extra else 0)


def streams_fast(f, w, h, a, b):
    """(luma words, chroma words, Y bytes, chroma bytes): does every row of the stream start 16-byte aligned (8 for halved chroma bytes)
    in every frame, with buffers that start aligned -- the kernel's rule for the 16-byte path of each stream (csrc/k_hdr.hip)"""
    lay, _, fb = PF.plane_layout(f, w, h, a)
    ocw, och = A.chroma_dims(w, h, b)
    pfb = A.frame_bytes(w, h, b)
    al = 8 if A.hshift(b) else 16
    return ((fb | lay[0][0] | lay[0][1]) % 16 == 0, all((fb | off | pitch) % 16 == 0 for off, pitch, _, _ in lay[1:]), (pfb | w) % 16 == 0,
            (pfb | (w * h) | (w * h + ocw * och) | ocw) % al == 0)


def check_geometry_list():
    """the list against the kernel's alignment rule, from the geometry alone: a self-check of this file's cases (it runs no product
    code), made where the cases are used"""
    for _, f, a, b in combos():
        assert streams_fast(fmt_for(f, 64, 16, a, 0, 0), 64, 16, a, b) == (True, True, True, True)           # every row on the vector path
        assert streams_fast(fmt_for(f, 160, 32, a, 0, 64), 160, 32, a, b) == (True, True, True, True)
        assert streams_fast(fmt_for(f, 48, 18, a, 3, 64), 48, 18, a, b)[:2] == (False, False)                  # pitch = row + 3: the byte path
        assert streams_fast(fmt_for(f, 48, 18, a, 16, 0), 48, 18, a, b)[:2] == (True, True)
    assert 17 % 16 == 1 and 33 % 16 == 1 and 15 < 16                     # tails of one pixel behind whole steps; no whole step
    assert A.chroma_dims(17, 5, S420) == (9, 3) and A.chroma_dims(15, 3, S420) == (8, 2)       # odd luma dims: both repeated edges
    assert (160 // 16) * (32 // 2) * 3 > 256 and len({g[3] for g in GEOMS}) == 2                 # more than one workgroup; n = 1 and n = 3
    assert {(a, b) for _, _, a, b in combos()} == set(HD.PAIRS)


def source(f, w, h, sub, n, seed):
    """sample values [n, samples of a frame] with codes 0 and the largest, and a peak white (index 4095: 2^20 of a PQ table)"""
    rng = np.random.default_rng(seed)
    top = (1 << f["depth"]) - 1
    vals = rng.integers(0, top + 1, (n, A.frame_bytes(w, h, sub)), dtype=np.uint32)
    cw, ch = A.chroma_dims(w, h, sub)
    for t in range(n):
        Y, U, V = PF._split(vals[t], w, h, sub)
        Y[0, 0], U[0, 0], V[0, 0] = top, top // 2 + 1, top // 2 + 1
        if w * h > 1:
            Y[-1, -1], U[-1, -1], V[-1, -1] = (0, 0, top) if t % 2 else (top, top, 0)
    return vals


@pytest.mark.parametrize("gi", range(len(GEOMS)))
def test_hdr_import_clip_equals_numpy(pkg, mem, tables, gi):
    """host memory for every case, twice with different padding bytes; device memory for every third: the source allocation and the
    256 guard bytes around the destination stay as they were"""
    check_geometry_list()
    w, h, pe, n, se = GEOMS[gi]
    ndev = 0
    for i, (name, f0, a, b) in enumerate(combos()):
        f = fmt_for(f0, w, h, a, pe, se)
        up = (i + gi) % 2
        tname, T, cT = tables[(i + 3 * gi) % len(tables)]
        vals = source(f, w, h, a, n, 7000 + 100 * gi + i)
        buf = PF.pack(vals, f, w, h, a, np.random.default_rng(1))
        want = HD.import_(buf, f, w, h, a, b, n, T, up)
        what = "%s %s 0x%x->0x%x %dx%d n=%d upsample %d tables %s" % (name, f, a, b, w, h, n, up, tname)
        got = pkg.hdr_import_clip(buf, cpf(pkg, f), w, h, a, b, cT, up)
        assert got.shape == want.shape
        assert np.array_equal(got, want), "host %s: first difference at %s" % (what, np.argwhere(got != want)[:3])
        other = PF.pack(vals, f, w, h, a, np.random.default_rng(2))
        if pe or se or f["msb"]:
            assert not np.array_equal(other, buf)
        assert np.array_equal(pkg.hdr_import_clip(other, cpf(pkg, f), w, h, a, b, cT, up), want), "host, other padding bytes, %s" % what
        if i % 3 != gi % 3:
            continue
        # the last frame may end with its planes
        short = buf[:(n - 1) * PF.frame_bytes(f, w, h, a) + PF.plane_layout(f, w, h, a)[1]]
        before = np.random.default_rng(3).integers(0, 256, GUARD + want.size + GUARD, dtype=np.uint8)
        src_d, dst_d = mem.alloc(short), mem.alloc(before)
        pkg.hdr_import_clip(src_d, cpf(pkg, f), w, h, a, b, cT, up, n=n, out=C.c_void_p(dst_d.value + GUARD))
        after = mem.read(dst_d, before.size)
        exp = before.copy()
        exp[GUARD:GUARD + want.size] = want.reshape(-1)
        assert np.array_equal(after, exp), "device %s: first difference at %s" % (what, np.argwhere(after != exp)[:3].ravel())
        assert np.array_equal(mem.read(src_d, short.size), short), "the source changed (%s)" % what
        ndev += 1
    assert ndev >= 8


def test_every_table_set_on_one_geometry(pkg, tables):
    """each curve and transfer, and the random tables, with both upsampling modes on P010"""
    w, h, n = 33, 6, 2
    f = FORMATS["P010"]
    buf = PF.pack(source(f, w, h, S420, n, 99), f, w, h, S420, np.random.default_rng(4))
    for name, T, cT in tables:
        for up in (RG.REPLICATE, RG.LINEAR):
            want = HD.import_(buf, f, w, h, S420, S420, n, T, up)
            got = pkg.hdr_import_clip(buf, cpf(pkg, f), w, h, S420, S420, cT, up)
            assert np.array_equal(got, want), (name, up, np.argwhere(got != want)[:3])


@pytest.mark.parametrize("w,h", [(64, 16), (17, 5)])
def test_import_at_a_subsampling_is_export_clip_of_the_444_import(pkg, tables, w, h):
    n = 2
    f = FORMATS["p10"]
    buf = PF.pack(source(f, w, h, S444, n, w), f, w, h, S444, np.random.default_rng(5))
    for name, T, cT in (tables[2], tables[-1]):
        full = pkg.hdr_import_clip(buf, cpf(pkg, f), w, h, S444, S444, cT, RG.LINEAR)
        for sub in (S422, S420):
            a = pkg.hdr_import_clip(buf, cpf(pkg, f), w, h, S444, sub, cT, RG.LINEAR)
            b = pkg.export_clip(full, w, h, S444, cpf(pkg, PF.pf()), sub)
            assert np.array_equal(a, b), (name, sub)


# ---- sessions --------------------------------------------------------------------------------------------------------------------
W, H, F, N = 64, 48, 4, 8
P010 = FORMATS["P010"]
GOP4 = dict(CRF, gop=4)


def hdr_clip(w, h, n, seed, style, f=P010, sub=S420):
    """a moving picture as an HDR clip of format f: a generated 8-bit clip widened to the depth, its low bits random, padded"""
    rng = np.random.default_rng(seed)
    c = A.gen_clip(w, h, sub, seed, n, style=style).astype(np.uint32)
    s = f["depth"] - 8
    vals = (c << s) | rng.integers(0, 1 << s, c.shape, dtype=np.uint32)
    g = fmt_for(f, w, h, sub, 32, 128)
    return PF.pack(vals, g, w, h, sub, rng).reshape(n, -1), g


def calls_of(clips, k):
    return [np.ascontiguousarray(np.stack([c[j * k:(j + 1) * k] for c in clips])) for j in range(clips[0].shape[0] // k)]


@pytest.fixture(scope="module")
def session_source(pkg, tables):
    """two sources: (raw clips, their format, the tables, hdr_import_clip's output of each): computed once"""
    _, _, cT = tables[2]
    raws, g = zip(*[hdr_clip(W, H, N, 0x4D0 + s, (0, 3)[s]) for s in range(2)])
    conv = [pkg.hdr_import_clip(r.reshape(-1), cpf(pkg, g[0]), W, H, S420, S420, cT, RG.LINEAR) for r in raws]
    assert conv[0].shape == (N, A.frame_bytes(W, H, S420)) and not np.array_equal(conv[0], conv[1])
    return list(raws), g[0], cT, conv


def with_hdr(pkg, make, g, cT, sub=None, up=RG.LINEAR):
    def go():
        b = make()
        b.set_source_hdr(cpf(pkg, g), cT, sub, up)
        return b
    return go


def test_batch_with_hdr_source(pkg, session_source):
    raws, g, cT, conv = session_source
    cfg = pkg.make_encoder_cfg(W, H, S420, **dict(GOP4, qp=80))
    want = run_batch(pkg, calls_of(conv, F), cfg, 2, F)
    assert all(len(x) > 0 for x in want)
    for mode, pipelined in [("host", True), ("device", True), ("held", True), ("host", False)]:
        got = run_batch(pkg, calls_of(raws, F), cfg, 2, F, mode=mode, pipelined=pipelined, opener=with_hdr(pkg, lambda: pkg.Batch(cfg, 2, F), g, cT))
        assert got == want, "%s pipelined=%s: not the stream of the converted clip" % (mode, pipelined)


def test_quality_ladder_and_chain_mode_with_hdr_source(pkg, session_source):
    raws, g, cT, conv = session_source
    rungs = [pkg.make_encoder_cfg(W, H, S420, **dict(GOP4, qp=q)) for q in (60, 90)]
    want = run_batch(pkg, calls_of(conv, F), None, 2, F, opener=lambda: pkg.Ladder(rungs, 2, F))
    assert len(want) == 4
    for mode in ("host", "held"):
        assert run_batch(pkg, calls_of(raws, F), None, 2, F, mode=mode, opener=with_hdr(pkg, lambda: pkg.Ladder(rungs, 2, F), g, cT)) == want, mode
    cfg = pkg.make_encoder_cfg(W, H, S420, **dict(GOP4, qp=75))
    want = run_batch(pkg, calls_of(conv[:1], N), cfg, 1, N, pipelined=False, opener=lambda: pkg.Batch(cfg, 1, N, chains=2))
    for mode in ("host", "device"):
        got = run_batch(pkg, calls_of(raws[:1], N), cfg, 1, N, mode=mode, pipelined=False, opener=with_hdr(pkg, lambda: pkg.Batch(cfg, 1, N, chains=2), g, cT))
        assert got == want, mode


def test_resolution_ladder_open_hdr(pkg, session_source):
    raws, g, cT, conv = session_source
    geoms = [(W, H, [dict(qp=80)]), (48, 32, [dict(qp=70)])]

    def ladder(**kw):
        return pkg.ResLadder(W, H, S420, [(gw, gh, [pkg.make_encoder_cfg(gw, gh, S420, **dict(GOP4, **r)) for r in rates]) for gw, gh, rates in geoms], 2, F, **kw)

    want = run_batch(pkg, calls_of(conv, F), None, 2, F, opener=ladder)
    assert len(want) == 4 and all(len(x) > 0 for x in want)
    for mode in ("host", "held"):
        b = ladder(src_format=cpf(pkg, g), src_hdr=cT)
        try:
            assert b.frame_bytes == PF.frame_bytes(g, W, H, S420)
            ins = [b.upload(c) for c in calls_of(raws, F)] if mode == "held" else calls_of(raws, F)
            got = [b""] * b.nstreams
            for c in ins:
                b.submit(c, on_device=mode == "held", held=mode == "held")
                got = [x + bytes(p) for x, p in zip(got, b.collect())]
            up = b.uploads()
        finally:
            b.close()
        assert got == want, mode
        assert up == ((raws[0].nbytes * 2, N // F) if mode == "host" else (0, 0))                 # the raw bytes
    meta = pkg.Meta()
    meta.width, meta.height, meta.subsamp = W, H, S420
    h_ = C.c_void_p(None)
    cfgs = (pkg.Encoder * 1)(pkg.make_encoder_cfg(W, H, S420, **dict(GOP4, qp=80)))
    rr = (pkg.ResRung * 1)(pkg.ResRung(W, H, 1, cfgs))
    L = pkg.lib()
    assert L.dsv1_resladder_open_hdr(C.byref(h_), C.byref(meta), C.byref(cpf(pkg, PF.pf(PF.PLANAR, 8, 0))), S420, C.byref(cT), 1, rr, 1, 0, 1, F, 1) == DSVG_ERR_ARG
    assert L.dsv1_resladder_open_hdr(C.byref(h_), C.byref(meta), C.byref(cpf(pkg, g)), S420, None, 1, rr, 1, 0, 1, F, 1) == DSVG_ERR_ARG
    assert L.dsv1_resladder_open_hdr(C.byref(h_), C.byref(meta), C.byref(cpf(pkg, g)), S420, C.byref(cT), 2, rr, 1, 0, 1, F, 1) == DSVG_ERR_ARG
    assert not h_.value


def test_hdr_with_levels_and_reframe(pkg, tables):
    """the HDR import in front of the levels and the reframe: 4:2:2 P210 frames of 80x40 halved to 4:2:0, cropped and padded to 64x48"""
    _, _, cT = tables[1]
    iw, ih = 80, 40
    raw, g = hdr_clip(iw, ih, N, 0x1E7, 1, FORMATS["P210"], S422)
    conv = pkg.hdr_import_clip(raw.reshape(-1), cpf(pkg, g), iw, ih, S422, S420, cT, RG.REPLICATE)
    rf = pkg.Reframe(iw, ih, window=(8, 0, 64, 40), out=(W, H), dst=(0, 4))
    lv = pkg.Levels.adjust(16, 235, 0, 255, 300)
    cfg = pkg.make_encoder_cfg(W, H, S420, **dict(GOP4, qp=80))

    def make(hdr):
        def go():
            b = pkg.Batch(cfg, 1, F)
            b.set_source_reframe(rf)
            if hdr:
                b.set_source_hdr(cpf(pkg, g), cT, S422, RG.REPLICATE)
            b.set_source_levels(lv)
            return b
        return go

    want = run_batch(pkg, calls_of([conv], F), cfg, 1, F, opener=make(False))
    for mode in ("host", "device"):
        assert run_batch(pkg, calls_of([raw], F), cfg, 1, F, mode=mode, opener=make(True)) == want, mode


def test_batch_error_contract_and_the_setters_replacing_each_other(pkg, session_source):
    raws, g, cT, conv = session_source
    L = pkg.lib()
    raw, clip = raws[0], conv[0]
    cfg = pkg.make_encoder_cfg(W, H, S420, **dict(GOP4, qp=80))
    want = run_batch(pkg, calls_of([clip], F), cfg, 1, F)[0]
    start = pkg.mem_outstanding()
    nv12 = PF.pf(PF.SEMI_UV)
    nv12_raw = PF.pack(clip, nv12, W, H, S420).reshape(N, -1)
    b = pkg.Batch(cfg, 1, F)
    try:
        planar_fb = b.frame_bytes
        hdr_fb = PF.frame_bytes(g, W, H, S420)
        pf, bad_t = cpf(pkg, g), pkg.HdrTables.from_dict(dict(cT.as_dict(), in_oy=-1))
        for args in [(cpf(pkg, PF.pf(PF.SEMI_UV, 8, 0)), S420, C.byref(cT), 1), (pf, S444, C.byref(cT), 1), (pf, A.SUBSAMP_411, C.byref(cT), 1),
                     (pf, S420, C.byref(cT), 2), (pf, S420, C.byref(bad_t), 1), (None, S420, C.byref(cT), 1)]:
            assert L.dsv1_batch_set_source_hdr(b.h, None if args[0] is None else C.byref(args[0]), *args[1:]) == DSVG_ERR_ARG, args[1:]
            assert b.frame_bytes == planar_fb
        b.set_source_format(cpf(pkg, nv12))              # replaced by the HDR setter ...
        b.set_source_hdr(pf, cT)
        assert b.frame_bytes == hdr_fb
        # an invalid call leaves the setting in force
        assert L.dsv1_batch_set_source_hdr(b.h, C.byref(pf), S420, C.byref(bad_t), 1) == DSVG_ERR_ARG
        assert b.frame_bytes == hdr_fb
        with pytest.raises(ValueError):
            b.submit(clip[:F][None])                     # the input-length check follows the format
        pin = b.pinned((1, F, raw.shape[1]))
        pin[...] = raw[:F][None]
        assert L.dsv1_batch_stage(b.h, pin.ctypes.data) == DSVG_ERR_ARG
        b.submit(pin)
        assert L.dsv1_batch_set_source_hdr(b.h, None, S420, None, 1) == DSVG_ERR_ARG                  # a batch in flight
        assert L.dsv1_batch_set_source_hdr(b.h, C.byref(pf), S420, C.byref(cT), 1) == DSVG_ERR_ARG
        assert b.frame_bytes == hdr_fb
        first = b.collect()[0]
        b.set_source_format(cpf(pkg, nv12))              # ... and the other way round: NV12 of the converted clip
        assert b.frame_bytes == PF.frame_bytes(nv12, W, H, S420)
        b.set_source_hdr(pf, cT)
        b.set_source_rgb(pkg.RgbFormat())                # the RGB setter replaces it too
        assert b.frame_bytes == 3 * W * H
        b.set_source_hdr(pf, cT)
        b.set_source_hdr(None, None)                     # NULL tables: back to packed planar
        assert b.frame_bytes == planar_fb and not L.dsv1_batch_has_source_lane(b.h)
        second = b.encode(clip[F:][None])[0]
        assert first + second == want
        # staged: refused, the setting stays as it was
        pin2 = b.pinned((1, F, clip.shape[1]))
        pin2[...] = clip[:F][None]
        b.stage(pin2)
        assert L.dsv1_batch_set_source_hdr(b.h, C.byref(pf), S420, C.byref(cT), 1) == DSVG_ERR_ARG
        assert b.frame_bytes == planar_fb
        b.submit(pin2)
        b.collect()
    finally:
        b.close()
    # (the context's memory: the converter's tables are a plain device allocation, which this counter does not see)
    assert pkg.mem_outstanding() == start
    assert L.dsv1_batch_set_source_hdr(None, None, S420, None, 1) == DSVG_ERR_ARG
