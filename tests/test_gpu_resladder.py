"""Resolution ladders (include/dsv1_api.h dsv1_resladder_*, Python ResLadder / encode_resolution_ladder): nsources sources, each scaled on
the GPU to several geometries and coded there at several rates, from one upload per call.  Output stream k = s * Ntot + off[g] + rate
must be byte for byte the oracle's stream of source s scaled by tests/_scale.py to geometry g, coded with that rate's settings, and its
per-picture SSE / SSIM the figures of the oracle's reconstructions against that scaled source."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import _scale as Z
import _ssim as Q

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return m


def expected(clip, recs, w, h, fmt, ssim):
    cw, ch = A.chroma_dims(w, h, fmt)
    sizes = [w * h, cw * ch, cw * ch]
    sse = np.zeros((len(recs), 3), dtype=np.uint64)
    fx = np.zeros((len(recs), 3), dtype=np.int64) if ssim else None
    for t, r in enumerate(recs):
        o = 0
        for p, n in enumerate(sizes):
            d = clip[t, o:o + n].astype(np.int64) - r[o:o + n].astype(np.int64)
            sse[t, p] = int((d * d).sum())
            o += n
        if ssim:
            fx[t] = Q.picture_fx(clip[t], r, w, h, fmt)
    return sse, fx


def oracle(clips, w, h, fmt, base, geoms, filt, ssim=True):
    """[k] = (stream bytes without EOS, SSE, SSIM_FX) in output order; geoms: [(gw, gh, [rate dicts])]"""
    out = []
    for clip in clips:
        for gw, gh, rates in geoms:
            sc = clip if (gw, gh) == (w, h) else Z.scale_clip(clip, w, h, fmt, gw, gh, filt)
            for rate in rates:
                data, recs = A.orc_encode(sc, A.orc_cfg(gw, gh, fmt, **dict(base, **rate)), want_recon=True, eos=False)
                out.append((data,) + expected(sc, recs, gw, gh, fmt, ssim))
    return out


def make(pkg, w, h, fmt, base, geoms, S, F, filt):
    return pkg.ResLadder(w, h, fmt, [(gw, gh, [pkg.make_encoder_cfg(gw, gh, fmt, **dict(base, **r)) for r in rates])
                                     for gw, gh, rates in geoms], S, F, filt)


def run(pkg, clips, w, h, fmt, base, geoms, F, filt=Z.CUBIC, mode="host", pipelined=True, streams=0, ssim=True):
    """code the clips in calls of F frames -> (streams, SSE [N, frames, 3], SSIM_FX or None, (upload bytes, upload calls))"""
    S, n = len(clips), clips[0].shape[0]
    assert n % F == 0
    b = make(pkg, w, h, fmt, base, geoms, S, F, filt)
    try:
        if streams:
            b.code_streams(streams)
        b.sse_enable()
        if ssim:
            b.ssim_enable()
        calls = [np.ascontiguousarray(np.stack([c[k * F:(k + 1) * F] for c in clips])) for k in range(n // F)]
        if mode in ("held", "device"):
            calls = [b.upload(c) for c in calls]
        elif mode == "pinned":
            pins = []
            for c in calls:
                p = b.pinned(c.shape)
                p[...] = c
                pins.append(p)
            calls = pins
        got, sse, fx = [b""] * b.nstreams, [], []
        dev = mode in ("held", "device")

        def take(part):
            assert len(part) == b.nstreams
            got[:] = [g + bytes(p) for g, p in zip(got, part)]
            sse.append(b.sse())
            if ssim:
                fx.append(b.ssim_fx())

        if pipelined:
            b.submit(calls[0], on_device=dev, held=mode == "held")
            for k in range(1, len(calls)):
                b.submit(calls[k], on_device=dev, held=mode == "held")
                take(b.collect())
            take(b.collect())
        else:
            for c in calls:
                take(b.encode(c, on_device=dev))
        up = b.uploads()
    finally:
        b.close()
    return got, np.concatenate(sse, axis=1), (np.concatenate(fx, axis=1) if ssim else None), up


def check(got, sse, fx, want):
    assert len(got) == len(want)
    for k, (data, esse, efx) in enumerate(want):
        assert got[k] == data, "output stream %d: packets differ from the oracle's" % k
        bad = np.nonzero((sse[k] != esse).any(axis=1))[0]
        assert bad.size == 0, "output stream %d: SSE differs at frames %s" % (k, bad[:4])
        if fx is not None:
            bad = np.nonzero((fx[k] != efx).any(axis=1))[0]
            assert bad.size == 0, "output stream %d: SSIM differs at frames %s" % (k, bad[:4])


FORMATS = [A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411]
CRF = dict(gop=12, rc_mode_cli=1, scd=1)


@pytest.mark.parametrize("fmt", FORMATS)
def test_formats(pkg, orc, fmt):
    """two sources (the second with scene cuts), three geometries at 1-2 CRF rates, 12 frames in calls of 6, pipelined"""
    w, h = 352, 288
    geoms = [(264, 216, [dict(qp=60), dict(qp=90)]), (176, 144, [dict(qp=80)]), (128, 96, [dict(qp=50), dict(qp=95)])]
    clips = [A.gen_clip(w, h, fmt, 0x5E5 + s, 12, style=(0, 3)[s]) for s in range(2)]
    got, sse, fx, _ = run(pkg, clips, w, h, fmt, CRF, geoms, 6)
    check(got, sse, fx, oracle(clips, w, h, fmt, CRF, geoms, Z.CUBIC))


@pytest.mark.parametrize("filt", [Z.TENT, Z.CUBIC])
def test_abr_both_filters(pkg, orc, filt):
    w, h, fmt = 352, 288, A.SUBSAMP_420
    base = dict(qp=80, gop=12, rc_mode_cli=0, scd=1)
    geoms = [(234, 192, [dict(kbps=300), dict(kbps=900)]), (118, 96, [dict(kbps=200)])]
    clips = [A.gen_clip(w, h, fmt, 0xAB5, 16, style=3)]
    got, sse, fx, _ = run(pkg, clips, w, h, fmt, base, geoms, 8, filt=filt)
    check(got, sse, fx, oracle(clips, w, h, fmt, base, geoms, filt))


@pytest.mark.parametrize("gop,F,n,style", [(0, 4, 8, 1), (30, 8, 24, 3)])
def test_gop_structures(pkg, orc, gop, F, n, style):
    """intra-only; a GOP longer than a call, with scene cuts"""
    w, h, fmt = 320, 240, A.SUBSAMP_420
    base = dict(gop=gop, rc_mode_cli=1, scd=1)
    geoms = [(240, 180, [dict(qp=70)]), (160, 120, [dict(qp=85), dict(qp=40)])]
    clips = [A.gen_clip(w, h, fmt, 0x60 + s, n, style=style) for s in range(2)]
    got, sse, fx, _ = run(pkg, clips, w, h, fmt, base, geoms, F, filt=Z.TENT)
    check(got, sse, fx, oracle(clips, w, h, fmt, base, geoms, Z.TENT))


def test_same_size_geometry_equals_a_plain_ladder(pkg, orc):
    w, h, fmt, F = 352, 288, A.SUBSAMP_420, 6
    rates = [dict(qp=55), dict(qp=90)]
    geoms = [(w, h, rates), (176, 144, [dict(qp=85)])]
    clips = [A.gen_clip(w, h, fmt, 0x5A5 + s, 12, style=s) for s in range(2)]
    got, sse, fx, _ = run(pkg, clips, w, h, fmt, CRF, geoms, F)
    check(got, sse, fx, oracle(clips, w, h, fmt, CRF, geoms, Z.CUBIC))
    b = pkg.Ladder([pkg.make_encoder_cfg(w, h, fmt, **dict(CRF, **r)) for r in rates], 2, F)
    try:
        lad = [b""] * 4
        for k in range(2):
            part = b.encode(np.stack([c[k * F:(k + 1) * F] for c in clips]))
            lad = [a + bytes(p) for a, p in zip(lad, part)]
    finally:
        b.close()
    assert [got[0], got[1], got[3], got[4]] == lad


@pytest.mark.parametrize("mode,pipelined", [("host", True), ("pinned", True), ("device", True), ("held", True), ("host", False),
                                            ("device", False)])
def test_input_forms(pkg, orc, mode, pipelined):
    """every input form over several calls; a same-size geometry among the scaled ones"""
    w, h, fmt, F = 256, 192, A.SUBSAMP_420, 4
    geoms = [(w, h, [dict(qp=80)]), (192, 144, [dict(qp=70)]), (96, 72, [dict(qp=90)])]
    clips = [A.gen_clip(w, h, fmt, 0xF0 + s, 16, style=s + 1) for s in range(2)]
    got, sse, fx, up = run(pkg, clips, w, h, fmt, CRF, geoms, F, mode=mode, pipelined=pipelined)
    check(got, sse, fx, oracle(clips, w, h, fmt, CRF, geoms, Z.CUBIC))
    fb = A.frame_bytes(w, h, fmt)
    if mode in ("host", "pinned"):
        assert up == (4 * 2 * F * fb, 4)               # one source clip per call, whatever the number of geometries
    else:
        assert up == (0, 0)


@pytest.mark.parametrize("streams", [1, 2])
def test_coding_streams(pkg, orc, streams):
    w, h, fmt = 352, 288, A.SUBSAMP_422
    geoms = [(300, 240, [dict(qp=75)]), (200, 160, [dict(qp=60), dict(qp=92)])]
    clips = [A.gen_clip(w, h, fmt, 0xC5 + s, 12, style=2) for s in range(3)]
    got, sse, fx, _ = run(pkg, clips, w, h, fmt, CRF, geoms, 6, streams=streams, ssim=False)
    check(got, sse, fx, oracle(clips, w, h, fmt, CRF, geoms, Z.CUBIC, ssim=False))


def test_1080p_to_720p_and_540p(pkg, orc):
    w, h, fmt = 1920, 1080, A.SUBSAMP_420
    geoms = [(1280, 720, [dict(qp=80)]), (960, 540, [dict(qp=70), dict(qp=90)])]
    clips = [A.gen_clip(w, h, fmt, 0x1080, 4, style=2)]
    got, sse, fx, _ = run(pkg, clips, w, h, fmt, CRF, geoms, 4, pipelined=False)
    check(got, sse, fx, oracle(clips, w, h, fmt, CRF, geoms, Z.CUBIC))


def test_encode_resolution_ladder(pkg, orc):
    w, h, fmt = 320, 180, A.SUBSAMP_420
    clip = A.gen_clip(w, h, fmt, 0xE1, 6, style=1)
    rungs = [dict(w=240, h=136, rates=[dict(qp=80), dict(qp=60)]), dict(w=160, h=90, rates=[dict(qp=85)])]
    got = pkg.encode_resolution_ladder(clip, w, h, fmt, rungs, gop=12)
    want = []
    for r in rungs:
        sc = Z.scale_clip(clip, w, h, fmt, r["w"], r["h"], Z.CUBIC)
        want += [A.orc_encode(sc, A.orc_cfg(r["w"], r["h"], fmt, **dict(gop=12, **q)))[0] for q in r["rates"]]
    assert got == want


def test_error_contract(pkg):
    w, h, fmt, F, S = 256, 192, A.SUBSAMP_420, 4, 2
    L = pkg.lib()
    geoms = [(192, 144, [dict(qp=50), dict(qp=90)]), (128, 96, [dict(qp=80)])]
    with pytest.raises(RuntimeError, match="rc=-2"):
        make(pkg, w, h, fmt, CRF, [(w * 2, h, [dict(qp=80)])], S, F, Z.CUBIC)
    with pytest.raises(RuntimeError, match="rc=-2"):
        make(pkg, w, h, fmt, CRF, geoms, S, F, 5)
    # a failure half way through the open (a host allocation of a ladder, after the scaler and that ladder's context exist) unwinds
    # everything and leaves no HIP error behind
    L.dsv1_debug_fail_alloc_at(3)
    try:
        with pytest.raises(RuntimeError):
            make(pkg, w, h, fmt, CRF, geoms, S, F, Z.CUBIC)
    finally:
        L.dsv1_debug_fail_alloc_at(0)
    b = make(pkg, w, h, fmt, CRF, geoms, S, F, Z.CUBIC)
    try:
        clip = np.stack([A.gen_clip(w, h, fmt, 0xE770 + s, F) for s in range(S)])
        with pytest.raises(ValueError):
            b.encode(np.concatenate([clip, clip]))
        out = b.encode(clip)
        assert len(out) == S * 3 == L.dsv1_resladder_nstreams(b.h)
        with pytest.raises(IndexError):
            b.encoder(S * 3)
        e = pkg.Buf()
        assert L.dsv1_resladder_eos(b.h, S * 3, C.byref(e)) == DSVG_ERR_ARG
        assert L.dsv1_resladder_collect(b.h, (pkg.Buf * (S * 3))()) == DSVG_ERR_ARG          # nothing in flight
        buf = (C.c_uint64 * (3 * F * S * 3))()
        assert L.dsv1_resladder_get_sse(b.h, buf, len(buf)) == DSVG_ERR_ARG                  # not measured
        b.sse_enable()
        b.encode(clip)
        assert L.dsv1_resladder_get_sse(b.h, buf, len(buf) - 1) == DSVG_ERR_ARG
        assert L.dsv1_resladder_get_sse(b.h, buf, len(buf)) == 0
        sse = np.frombuffer(buf, dtype=np.uint64).reshape(S * 3, F, 3)
        assert (sse[0::3].sum(axis=-1) > sse[1::3].sum(axis=-1)).all()      # qp 50 against qp 90 at the same geometry
        assert b.eos(0)[5] == 0x10
        assert b.psnr().shape == (S * 3, F, 4) and b.stream_dims(2) == (128, 96)
    finally:
        b.close()
    # and a plain ladder opens and codes as ever after all of it
    out = pkg.encode_ladder(A.gen_clip(176, 144, fmt, 0x11, 4), 176, 144, fmt, [dict(qp=80)], gop=12)
    assert out[0] == A.orc_encode(A.gen_clip(176, 144, fmt, 0x11, 4), A.orc_cfg(176, 144, fmt, qp=80, gop=12))[0]
