"""Resolution-ladder rungs measured at the SOURCE resolution (include/dsv1_api.h dsv1_resladder_src_quality_enable / get_src_*,
csrc/k_quality.hip k_xres_quality): every picture's reconstruction upscaled to the source's dims by tests/_resample.py and compared
with the original source must give the device's SSE and SSIM_FX to the integer, the packets must not change, and the source must
be held until collect in every input form."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import _resample as RS
import _scale as Z

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2
FORMATS = [A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411]
CRF = dict(gop=12, rc_mode_cli=1, scd=1)


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return m


def oracle(clips, w, h, fmt, base, geoms, filt, sfilt):
    """[k] = (stream bytes without EOS, source-resolution SSE [n, 3], SSIM_FX [n, 3]) in output order"""
    out = []
    for clip in clips:
        for gw, gh, rates in geoms:
            sc = clip if (gw, gh) == (w, h) else Z.scale_clip(clip, w, h, fmt, gw, gh, filt)
            for rate in rates:
                data, recs = A.orc_encode(sc, A.orc_cfg(gw, gh, fmt, **dict(base, **rate)), want_recon=True, eos=False)
                q = [RS.src_quality(clip[t], r, w, h, gw, gh, fmt, sfilt) for t, r in enumerate(recs)]
                out.append((data, np.stack([a for a, _ in q]), np.stack([b for _, b in q])))
    return out


def make(pkg, w, h, fmt, base, geoms, S, F, filt):
    return pkg.ResLadder(w, h, fmt, [(gw, gh, [pkg.make_encoder_cfg(gw, gh, fmt, **dict(base, **r)) for r in rates])
                                     for gw, gh, rates in geoms], S, F, filt)


def run(pkg, clips, w, h, fmt, base, geoms, F, filt=Z.CUBIC, sfilt=Z.CUBIC, mode="host", pipelined=True, xsse=True, xssim=True,
        rung=False, clobber=False):
    """code the clips in calls of F frames -> (streams, src SSE, src SSIM_FX, rung SSE, rung SSIM_FX) ([N, frames, 3] or None)"""
    S, n = len(clips), clips[0].shape[0]
    b = make(pkg, w, h, fmt, base, geoms, S, F, filt)
    try:
        if xsse or xssim:
            b.src_quality_enable(sse=xsse, ssim=xssim, filt=sfilt)
        if rung:
            b.sse_enable()
            b.ssim_enable()
        calls = [np.ascontiguousarray(np.stack([c[k * F:(k + 1) * F] for c in clips])) for k in range(n // F)]
        dev = mode in ("held", "device")
        if dev:
            calls = [b.upload(c) for c in calls]
        elif mode == "pinned":
            pins = []
            for c in calls:
                p = b.pinned(c.shape)
                p[...] = c
                pins.append(p)
            calls = pins
        got, res = [b""] * b.nstreams, [[], [], [], []]
        junk = np.full(S * F * A.frame_bytes(w, h, fmt), 0x5A, dtype=np.uint8)

        def take(part):
            got[:] = [g + bytes(p) for g, p in zip(got, part)]
            for i, (on, f) in enumerate([(xsse, b.src_sse), (xssim, b.src_ssim_fx), (rung, b.sse), (rung, b.ssim_fx)]):
                if on:
                    res[i].append(f())

        def submit(c):
            b.submit(c, on_device=dev, held=mode == "held")
            if clobber:                              # a plain device clip is the caller's again when submit returns
                assert b.L.dsvg_dev_upload(b.ctx, c, junk.ctypes.data, junk.nbytes) == 0

        if pipelined:
            submit(calls[0])
            for k in range(1, len(calls)):
                submit(calls[k])
                take(b.collect())
            take(b.collect())
        else:
            for c in calls:
                take(b.encode(c, on_device=dev))
    finally:
        b.close()
    return (got,) + tuple(np.concatenate(r, axis=1) if r else None for r in res)


def check(got, sse, fx, want):
    assert len(got) == len(want)
    for k, (data, esse, efx) in enumerate(want):
        assert got[k] == data, "output stream %d: packets differ from the oracle's" % k
        if sse is not None:
            bad = np.nonzero((sse[k] != esse).any(axis=1))[0]
            assert bad.size == 0, "output stream %d: source-resolution SSE differs at frames %s: %s vs %s" % (
                k, bad[:4], sse[k][bad[0]], esse[bad[0]])
        if fx is not None:
            bad = np.nonzero((fx[k] != efx).any(axis=1))[0]
            assert bad.size == 0, "output stream %d: source-resolution SSIM differs at frames %s: %s vs %s" % (
                k, bad[:4], fx[k][bad[0]], efx[bad[0]])


@pytest.mark.parametrize("fmt", FORMATS)
def test_formats(pkg, orc, fmt):
    """two sources (the second with scene cuts), a same-size geometry and two smaller ones, CRF, 8 frames in calls of 4, pipelined"""
    w, h = 176, 144
    geoms = [(w, h, [dict(qp=80)]), (128, 96, [dict(qp=60), dict(qp=90)]), (96, 72, [dict(qp=70)])]
    clips = [A.gen_clip(w, h, fmt, 0x7E5 + s, 8, style=(0, 3)[s]) for s in range(2)]
    got, sse, fx, _, _ = run(pkg, clips, w, h, fmt, CRF, geoms, 4)
    check(got, sse, fx, oracle(clips, w, h, fmt, CRF, geoms, Z.CUBIC, Z.CUBIC))


@pytest.mark.parametrize("filt,sfilt", [(Z.TENT, Z.TENT), (Z.CUBIC, Z.TENT), (Z.TENT, Z.CUBIC)])
def test_abr_both_filters(pkg, orc, filt, sfilt):
    w, h, fmt = 176, 144, A.SUBSAMP_420
    base = dict(qp=80, gop=12, rc_mode_cli=0, scd=1)
    geoms = [(118, 96, [dict(kbps=150), dict(kbps=400)]), (96, 72, [dict(kbps=80)])]
    clips = [A.gen_clip(w, h, fmt, 0xAB6, 8, style=3)]
    got, sse, fx, _, _ = run(pkg, clips, w, h, fmt, base, geoms, 4, filt=filt, sfilt=sfilt)
    check(got, sse, fx, oracle(clips, w, h, fmt, base, geoms, filt, sfilt))


@pytest.mark.parametrize("gop,F,n,style", [(0, 4, 8, 1), (30, 4, 12, 3)])
def test_gop_structures(pkg, orc, gop, F, n, style):
    """intra-only (no picture keeps its reconstruction otherwise); a GOP longer than a call with scene cuts; SSE and SSIM alone"""
    w, h, fmt = 320, 240, A.SUBSAMP_420
    base = dict(gop=gop, rc_mode_cli=1, scd=1)
    geoms = [(240, 180, [dict(qp=70)]), (160, 120, [dict(qp=85)])]
    clips = [A.gen_clip(w, h, fmt, 0x61 + s, n, style=style) for s in range(2)]
    want = oracle(clips, w, h, fmt, base, geoms, Z.TENT, Z.CUBIC)
    got, sse, _, _, _ = run(pkg, clips, w, h, fmt, base, geoms, F, filt=Z.TENT, xssim=False)
    check(got, sse, None, want)
    got, _, fx, _, _ = run(pkg, clips, w, h, fmt, base, geoms, F, filt=Z.TENT, xsse=False)
    check(got, None, fx, want)


def test_packets_identical_on_and_off(pkg):
    w, h, fmt = 192, 144, A.SUBSAMP_420
    geoms = [(w, h, [dict(qp=75)]), (128, 96, [dict(qp=60), dict(qp=90)])]
    clips = [A.gen_clip(w, h, fmt, 0x0F + s, 8, style=s + 1) for s in range(2)]
    off = run(pkg, clips, w, h, fmt, CRF, geoms, 4, xsse=False, xssim=False)[0]
    on = run(pkg, clips, w, h, fmt, CRF, geoms, 4, rung=True)[0]
    assert on == off


@pytest.mark.parametrize("mode,pipelined,clobber", [("host", True, False), ("pinned", True, False), ("device", True, True),
                                                    ("held", True, False), ("host", False, False), ("device", False, True)])
def test_input_forms(pkg, orc, mode, pipelined, clobber):
    """every input form over several calls; a plain device clip overwritten as soon as submit returns still gives its figures"""
    w, h, fmt, F = 256, 192, A.SUBSAMP_420, 4
    geoms = [(w, h, [dict(qp=80)]), (192, 144, [dict(qp=70)]), (96, 72, [dict(qp=90)])]
    clips = [A.gen_clip(w, h, fmt, 0xF7 + s, 12, style=s + 1) for s in range(2)]
    got, sse, fx, _, _ = run(pkg, clips, w, h, fmt, CRF, geoms, F, mode=mode, pipelined=pipelined, clobber=clobber)
    check(got, sse, fx, oracle(clips, w, h, fmt, CRF, geoms, Z.CUBIC, Z.CUBIC))


@pytest.mark.parametrize("sfilt", [Z.TENT, Z.CUBIC])
def test_same_size_geometry_equals_rung_figures(pkg, sfilt):
    """a geometry of the source's size goes through the identity tables: its figures are get_sse / get_ssim's"""
    w, h, fmt = 176, 144, A.SUBSAMP_422
    geoms = [(w, h, [dict(qp=50), dict(qp=90)]), (128, 96, [dict(qp=80)])]
    clips = [A.gen_clip(w, h, fmt, 0x55 + s, 8, style=2) for s in range(2)]
    _, sse, fx, rsse, rfx = run(pkg, clips, w, h, fmt, CRF, geoms, 4, sfilt=sfilt, rung=True)
    same = [k for k in range(len(sse)) if k % 3 < 2]
    assert np.array_equal(sse[same], rsse[same]) and np.array_equal(fx[same], rfx[same])
    assert (sse[2::3].sum(axis=-1) > rsse[2::3].sum(axis=-1)).all()      # the smaller rung loses what the downscale threw away


def test_1080p_with_720p_and_540p_rungs(pkg, orc):
    w, h, fmt = 1920, 1080, A.SUBSAMP_420
    geoms = [(1280, 720, [dict(qp=80)]), (960, 540, [dict(qp=70)])]
    clips = [A.gen_clip(w, h, fmt, 0x1081, 2, style=2)]
    got, sse, fx, _, _ = run(pkg, clips, w, h, fmt, CRF, geoms, 2, pipelined=False)
    check(got, sse, fx, oracle(clips, w, h, fmt, CRF, geoms, Z.CUBIC, Z.CUBIC))


def test_error_contract(pkg):
    w, h, fmt, F, S = 256, 192, A.SUBSAMP_420, 4, 2
    L = pkg.lib()
    geoms = [(192, 144, [dict(qp=50), dict(qp=90)]), (128, 96, [dict(qp=80)])]
    b = make(pkg, w, h, fmt, CRF, geoms, S, F, Z.CUBIC)
    try:
        clip = np.stack([A.gen_clip(w, h, fmt, 0xE771 + s, F) for s in range(S)])
        n = 3 * F * S * 3
        buf, fxb = (C.c_uint64 * n)(), (C.c_int64 * n)()
        for f in (-1, 2, 9):
            assert L.dsv1_resladder_src_quality_enable(b.h, 1, 1, f) == DSVG_ERR_ARG
        b.encode(clip)
        assert L.dsv1_resladder_get_src_sse(b.h, buf, n) == DSVG_ERR_ARG              # not measured
        assert L.dsv1_resladder_get_src_ssim(b.h, fxb, n) == DSVG_ERR_ARG
        b.submit(clip)
        assert L.dsv1_resladder_src_quality_enable(b.h, 1, 1, 1) == DSVG_ERR_ARG      # a call in flight
        b.collect()
        b.src_quality_enable()
        b.encode(clip)
        assert L.dsv1_resladder_get_src_sse(b.h, buf, n - 1) == DSVG_ERR_ARG
        assert L.dsv1_resladder_get_src_ssim(b.h, fxb, n - 1) == DSVG_ERR_ARG
        assert L.dsv1_resladder_get_src_sse(b.h, buf, n) == 0 and L.dsv1_resladder_get_src_ssim(b.h, fxb, n) == 0
        with pytest.raises(RuntimeError, match="rc=-2"):
            b.sse()                                                                  # the rung-resolution pair is independent
        assert b.src_psnr().shape == (S * 3, F, 4) and b.src_ssim().shape == (S * 3, F, 4)
        p = b.src_psnr()
        assert (p[0::3, :, 3] < p[1::3, :, 3]).all()                                 # qp 50 against qp 90 at the same geometry
        s = b.src_ssim()
        assert np.isfinite(s).all() and (s <= 1.0).all()
        b.src_quality_enable(False, False)
        b.encode(clip)
        assert L.dsv1_resladder_get_src_sse(b.h, buf, n) == DSVG_ERR_ARG              # switched off again
    finally:
        b.close()


def test_all_four_kinds_switched_from_call_to_call(pkg, orc):
    """rung SSE / SSIM and source-resolution SSE / SSIM on one resolution ladder, another setting every two calls (all on; rung SSIM
    and source SSE; all off; rung SSE and source SSIM), the two calls of a setting in flight together so that both halves of the
    out slots carry it: after every collect a kind that is on gives the oracle's figures of those frames, one that is off is refused
    by its getter, and the packets are the oracle's"""
    from test_gpu_quality import expected_sse
    from test_gpu_ssim import expected as expected_ssim
    w, h, fmt, F, n = 176, 144, A.SUBSAMP_420, 4, 32
    geoms = [(w, h, [dict(qp=80)]), (96, 72, [dict(qp=60), dict(qp=90)])]
    clips = [A.gen_clip(w, h, fmt, 0x4C1 + s, n, style=(0, 3)[s]) for s in range(2)]
    want = [[], [], [], [], []]                      # streams, then the kinds in the getters' order below: [N][n, 3]
    for clip in clips:
        for gw, gh, rates in geoms:
            sc = clip if (gw, gh) == (w, h) else Z.scale_clip(clip, w, h, fmt, gw, gh, Z.CUBIC)
            for rate in rates:
                data, recs = A.orc_encode(sc, A.orc_cfg(gw, gh, fmt, **dict(CRF, **rate)), want_recon=True, eos=False)
                q = [RS.src_quality(clip[t], r, w, h, gw, gh, fmt, Z.CUBIC) for t, r in enumerate(recs)]
                for i, v in enumerate([data, expected_sse(sc, recs, gw, gh, fmt), expected_ssim(sc, recs, gw, gh, fmt)[0],
                                       np.stack([a for a, _ in q]), np.stack([x for _, x in q])]):
                    want[i].append(v)
    b = make(pkg, w, h, fmt, CRF, geoms, 2, F, Z.CUBIC)
    try:
        L, N = b.L, b.nstreams
        kinds = [(L.dsv1_resladder_get_sse, C.c_uint64), (L.dsv1_resladder_get_ssim, C.c_int64),
                 (L.dsv1_resladder_get_src_sse, C.c_uint64), (L.dsv1_resladder_get_src_ssim, C.c_int64)]
        got, call = [b""] * N, 0
        calls = [np.ascontiguousarray(np.stack([c[k * F:(k + 1) * F] for c in clips])) for k in range(n // F)]

        def take(on):
            nonlocal call
            got[:] = [g + bytes(p) for g, p in zip(got, b.collect())]
            for i, (get, ty) in enumerate(kinds):
                buf = np.zeros((N, F, 3), dtype=ty)
                rc = get(b.h, buf.ctypes.data_as(C.POINTER(ty)), buf.size)
                if not on[i]:
                    assert rc == DSVG_ERR_ARG, "call %d: kind %d is off and was delivered (rc %d)" % (call, i, rc)
                    continue
                assert rc == 0, "call %d: kind %d is on, rc %d" % (call, i, rc)
                exp = np.stack([v[call * F:(call + 1) * F] for v in want[1 + i]])
                assert np.array_equal(buf, exp), "call %d: kind %d differs from the oracle's in streams %s" % (
                    call, i, sorted(set(np.nonzero(buf != exp)[0])))
            call += 1

        for on in [(1, 1, 1, 1), (0, 1, 1, 0), (0, 0, 0, 0), (1, 0, 0, 1)]:
            b.sse_enable(on[0])
            b.ssim_enable(on[1])
            b.src_quality_enable(sse=on[2], ssim=on[3], filt=Z.CUBIC)
            b.submit(calls[call])
            b.submit(calls[call + 1])
            take(on)
            take(on)
    finally:
        b.close()
    assert call == n // F
    for k in range(N):
        assert got[k] == want[0][k], "output stream %d: packets differ from the oracle's" % k


def test_nothing_measured_logs_nothing(pkg, capfd):
    """a resolution ladder with no measurement on gathers no figures and asks for none: a call logs no "not measured" line (the
    library logs to stdout; the refused getter after the call shows that the capture sees its lines)"""
    w, h, fmt, F = 176, 144, A.SUBSAMP_420, 4
    libc = C.CDLL(None)
    b = make(pkg, w, h, fmt, CRF, [(w, h, [dict(qp=80)]), (96, 72, [dict(qp=60), dict(qp=90)])], 1, F, Z.CUBIC)
    try:
        libc.fflush(None)
        capfd.readouterr()
        b.encode(A.gen_clip(w, h, fmt, 0x109, F).reshape(1, F, -1))
        libc.fflush(None)
        out = capfd.readouterr().out
        assert "not measured" not in out and "nothing measured" not in out, out
        buf = (C.c_uint64 * (3 * F * 3))()
        assert b.L.dsv1_resladder_get_sse(b.h, buf, len(buf)) == DSVG_ERR_ARG
        libc.fflush(None)
        assert "dsv1_resladder_get_sse: nothing measured" in capfd.readouterr().out
    finally:
        b.close()
