"""Decoder output scale on the GPU (include/dsv1_api.h, decoder output scale; csrc/k_scale.hip k_scale_slots; the output pass of
csrc/dsvg_pipe.hip).  Everything is exact: the definition is tests/_resample.py applied to the decoded frames at the stream's
subsampling, followed by tests/_pixout.py, _chroma.py or _rgb.py at the scaled geometry; every comparison is byte equality over the
whole output buffer, with a random sentinel in everything the pass must not write."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import _chroma as CH
import _pixfmt as PF
import _pixout as PO
import _resample as RS
import _rgb as RG
import outscale_cases as OC
from test_gpu_decode_escape import _two_picture_stream, plane_payload, region_base, splice
from test_gpu_drawinfo import decoder_case, run as run_drawn
from test_gpu_pixfmt import padded
from test_gpu_pixout import cpf, streams_of
from test_gpu_rgb import crf

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2
S420, S422, S444 = OC.S420, OC.S422, OC.S444
FILTERS = [RS.TENT, RS.CUBIC]


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return m


_scaled = {}


def scaled(key, frame, w, h, fmt, dw, dh, filt):
    """the definition of one frame, computed once per (key, target, filter) and never modified"""
    k = (key, w, h, fmt, dw, dh, filt)
    if k not in _scaled:
        _scaled[k] = RS.resample_frame(frame, w, h, fmt, dw, dh, filt)
        _scaled[k].setflags(write=False)
    return _scaled[k]


# ---- 1. context level, hostile borders ------------------------------------------------------------------------------------------
def bordered_frames(w, h, fmt, n, rng):
    """n frames in the reference layout (csrc/dsvg_common.hip make_frame_layout: Y, U, V back to back, 64-pixel borders, rows of
    round16(width + 128)) whose every byte is random -- the borders are NOT the replicated edge -- and their picture areas as packed
    planar frames"""
    raws, pics, off = [], [], 0
    lay = []
    for pw, ph in OC.plane_dims(w, h, fmt):
        stride = (pw + 128 + 15) & ~15
        lay.append((off, stride, pw, ph))
        off += stride * (ph + 128)
    for _ in range(n):
        raw = rng.integers(0, 256, off, dtype=np.uint8)
        pic = []
        for o, stride, pw, ph in lay:
            pl = raw[o:o + stride * (ph + 128)].reshape(ph + 128, stride)
            pic.append(pl[64:64 + ph, 64:64 + pw].reshape(-1))
        raws.append(raw)
        pics.append(np.concatenate(pic))
    return raws, pics, off


@pytest.mark.parametrize("w,h,fmt", sorted(OC.CTX_TARGETS))
def test_context_scales_slots_with_hostile_borders(pkg, w, h, fmt):
    """the kernel clamps and never reads the border: slots whose borders hold noise give the definition of the picture area"""
    L = pkg.lib()
    L.dsvg_ctx_create.argtypes = [C.POINTER(C.c_void_p)] + [C.c_int] * 9
    L.dsvg_ctx_destroy.argtypes = [C.c_void_p]
    L.dsvg_ctx_destroy.restype = None
    L.dsvg_upload_recon_raw.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.dsvg_pack_recons.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_size_t, C.c_int]
    L.dsvg_ctx_sync.argtypes = [C.c_void_p]
    L.dsvg_last_error.restype = C.c_char_p
    slots = [4, 0, 2, 5, 1]
    n = len(slots)
    rng = np.random.default_rng(w * 131 + h)
    raws, pics, raw_bytes = bordered_frames(w, h, fmt, n, rng)
    ctx = C.c_void_p(None)
    assert L.dsvg_ctx_create(C.byref(ctx), 0, w, h, fmt, 1, 1, 6, 2, 2) == 0, L.dsvg_last_error()
    dev = C.c_void_p(None)
    try:
        for i, s in enumerate(slots):
            assert L.dsvg_upload_recon_raw(ctx, s, raws[i].ctypes.data, raw_bytes) == 0, L.dsvg_last_error()
        tab = (C.c_int * n)(*slots)
        cap = n * (A.frame_bytes(8 * w, 8 * h, fmt) // 16 + 64)
        assert L.dsvg_dev_alloc(ctx, C.byref(dev), cap) == 0
        cases = [(t, f) for t in OC.CTX_TARGETS[(w, h, fmt)] for f in FILTERS] + [(None, RS.CUBIC)]      # last: switched off again
        for (target, filt) in cases:
            dw, dh = target or (w, h)
            if target:
                assert L.dsvg_ctx_output_scale(ctx, dw, dh, filt) == 0, L.dsvg_last_error()
                want = [scaled(("ctx", i), pics[i], w, h, fmt, dw, dh, filt) for i in range(n)]
            else:
                assert L.dsvg_ctx_output_scale(ctx, 0, 0, filt) == 0
                want = pics
            fb = A.frame_bytes(dw, dh, fmt)
            pitch = fb + 37                              # (frames at odd addresses, and bytes between them that stay)
            assert n * pitch <= cap
            expect = rng.integers(0, 256, n * pitch, dtype=np.uint8)
            host = expect.copy()
            assert L.dsvg_dev_upload(ctx, dev, expect.ctypes.data, expect.nbytes) == 0
            for i in range(n):
                expect[i * pitch:i * pitch + fb] = want[i]
            what = "%dx%d -> %dx%d filter %d" % (w, h, dw, dh, filt)
            assert L.dsvg_pack_recons(ctx, n, tab, host.ctypes.data, pitch, 0) == 0, L.dsvg_last_error()
            assert np.array_equal(host, expect), "host, %s: first difference at %s" % (what, np.argwhere(host != expect)[:3].ravel())
            assert L.dsvg_pack_recons(ctx, n, tab, dev, pitch, 1) == 0, L.dsvg_last_error()
            assert L.dsvg_ctx_sync(ctx) == 0
            got = np.zeros(n * pitch, dtype=np.uint8)
            assert L.dsvg_dev_download(ctx, got.ctypes.data, dev, got.nbytes) == 0
            assert np.array_equal(got, expect), "device, %s: first difference at %s" % (what, np.argwhere(got != expect)[:3].ravel())
            if target:                                   # a frame smaller than the pitch asks for is refused, nothing written
                assert L.dsvg_pack_recons(ctx, n, tab, host.ctypes.data, fb - 1, 0) == DSVG_ERR_ARG
                assert np.array_equal(host, expect)
        # refusals leave the setting in force: the list's second target, tent, stays what the pass does
        dw, dh = OC.CTX_TARGETS[(w, h, fmt)][1]
        assert L.dsvg_ctx_output_scale(ctx, dw, dh, RS.TENT) == 0
        for bad in [(8 * w + 1, h, RS.TENT), (w, 8 * h + 1, RS.TENT), (w, (h - 1) // 8, RS.CUBIC), (dw, dh, 2), (dw, dh, -1), (0, dh, RS.TENT), (dw, -1, RS.TENT)]:
            assert L.dsvg_ctx_output_scale(ctx, *bad) == DSVG_ERR_ARG, bad
        fb = A.frame_bytes(dw, dh, fmt)
        host = np.zeros((n, fb), dtype=np.uint8)
        assert L.dsvg_pack_recons(ctx, n, tab, host.ctypes.data, fb, 0) == 0, L.dsvg_last_error()
        for i in range(n):
            assert np.array_equal(host[i], scaled(("ctx", i), pics[i], w, h, fmt, dw, dh, RS.TENT)), i
    finally:
        if dev:
            L.dsvg_dev_free(ctx, dev)
        L.dsvg_ctx_destroy(ctx)


# ---- the batched decoder -------------------------------------------------------------------------------------------------------
def planar(fmt):
    """the setting without a format: packed planar frames of the scaled geometry"""
    return dict(apply=None, fb=lambda dw, dh: A.frame_bytes(dw, dh, fmt), frame=lambda x, dw, dh, into: into.__setitem__(slice(None), x))


def run_scaled(pkg, packets, full, w, h, fmt, S, plan, on_device, seed=3):
    """tests/test_gpu_pixout.py run_decoder with a scale in the setting: plan(call) -> dict(name, scale=(dw, dh, filter) or None,
    pre=callable(pkg, d) or None, out=dict(apply, fb, frame)).  A change of name sets the scale FIRST and the format SECOND.  After every call
    the whole output buffer is compared with a host copy into which the expected bytes of the streams that had a picture were written;
    the other streams' frames and every padding byte keep the sentinel.  full(s, t): the full-size frame of stream s, picture t"""
    L = pkg.lib()
    d = pkg.DecBatch(w, h, fmt, S)
    try:
        eos = bytes(packets[0][-1])
        count = [0] * S
        cur, expect, dev, host, fb = None, None, None, None, 0
        for k in range(max(len(p) for p in packets)):
            st = plan(k)
            if st["name"] != cur:
                cur = st["name"]
                if st.get("pre"):
                    st["pre"](pkg, d)
                sc = st["scale"]
                if sc:
                    d.set_output_scale(*sc)
                else:
                    d.set_output_scale(None)
                dw, dh = sc[:2] if sc else (w, h)
                assert d.out_dims == (dw, dh)
                assert d.frame_bytes == A.frame_bytes(dw, dh, fmt) == L.dsv1_decbatch_out_frame_bytes(d.h)     # the format is dropped
                out = st["out"]
                if out["apply"]:
                    out["apply"](pkg, d, dw, dh)
                fb = out["fb"](dw, dh)
                assert d.frame_bytes == fb == L.dsv1_decbatch_out_frame_bytes(d.h) and d.out_dims == (dw, dh)
                expect = np.random.default_rng(seed + k).integers(0, 256, S * fb, dtype=np.uint8)     # the sentinel
                if on_device:
                    dev = d.dev_alloc()
                    assert d.L.dsvg_dev_upload(d.ctx, dev, expect.ctypes.data, expect.nbytes) == 0
                else:
                    host = expect.copy().reshape(S, fb)
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
                    x = full(s, count[s])
                    if st["scale"]:
                        x = scaled(("dec", s, count[s]), x, w, h, fmt, *st["scale"])
                    st["out"]["frame"](x, dw, dh, expect[s * fb:(s + 1) * fb])
                    count[s] += 1
                else:
                    assert status[s] in (2, 3)
            assert np.array_equal(got, expect), "call %d (%s): first difference at byte %s of %d-byte frames" % (
                k, cur, np.argwhere(got != expect)[:3].ravel(), fb)
        return count
    finally:
        d.close()


DEC_CASES = [(g, t, f) for g in sorted(OC.DEC_TARGETS) for t in OC.DEC_TARGETS[g] for f in FILTERS]


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("geom,target,filt", DEC_CASES, ids=["%dx%d-0x%x-%dx%d-f%d" % (g + t + (f,)) for g, t, f in DEC_CASES])
def test_batched_decoder_packed_planar(pkg, orc, geom, target, filt, on_device):
    """four streams with mixed GOPs; some calls leave a stream without a picture (its frame keeps the sentinel); P pictures of later
    calls still equal the oracle's, so the references stayed at full size and clean"""
    w, h, fmt = geom
    _, packets, want = streams_of(w, h, fmt)
    assert any(len(p) != len(packets[0]) for p in packets)
    st = dict(name="scaled", scale=target + (filt,), out=planar(fmt))
    count = run_scaled(pkg, packets, lambda s, t: want[s][t], w, h, fmt, 4, lambda k: st, on_device)
    assert count == [len(x) for x in want]


def nv12(fmt, pad=None, depth=8):
    def f_of(dw, dh):
        f = PF.pf(PF.SEMI_UV, depth, 1 if depth > 8 else 0)
        return padded(f, dw, dh, S420, **pad) if pad else f
    return dict(apply=lambda pkg, d, dw, dh: d.set_output_format(cpf(pkg, f_of(dw, dh)), S420),
                fb=lambda dw, dh: PF.frame_bytes(f_of(dw, dh), dw, dh, S420),
                frame=lambda x, dw, dh, into: PO.export(x[None], f_of(dw, dh), dw, dh, fmt, S420, 1, into=into))


def yuyv422(fmt):
    f = PF.pf(PF.YUYV)
    return dict(apply=lambda pkg, d, dw, dh: d.set_output_format(cpf(pkg, f), S422), fb=lambda dw, dh: PF.frame_bytes(f, dw, dh, S422),
                frame=lambda x, dw, dh, into: PO.export(x[None], f, dw, dh, fmt, S422, 1, into=into))


def planar444_linear(fmt):
    f = PF.pf()
    return dict(apply=lambda pkg, d, dw, dh: d.set_output_format(cpf(pkg, f), S444, upsample=pkg.CHROMA_LINEAR),
                fb=lambda dw, dh: PF.frame_bytes(f, dw, dh, S444),
                frame=lambda x, dw, dh, into: CH.export_up(x[None], f, dw, dh, fmt, S444, CH.LINEAR, 1, into=into))


def rgb24(fmt):
    f = RG.rf(RG.RGB24, RG.BT709)
    return dict(apply=lambda pkg, d, dw, dh: d.set_output_rgb(crf(pkg, f)), fb=lambda dw, dh: RG.frame_bytes(f, dw, dh),
                frame=lambda x, dw, dh, into: RG.export(x[None], f, dw, dh, fmt, 1, into=into))


FORMATS = {
    "nv12":             ((352, 288, S420), (176, 144), RS.CUBIC, nv12),
    "nv12-odd-up":      ((352, 288, S420), (399, 301), RS.TENT, nv12),
    "p010-padded":      ((352, 288, S420), (176, 144), RS.TENT, lambda fmt: nv12(fmt, dict(pad=(48, 16, 80), stride_pad=256), 10)),
    "p010-padded-odd":  ((352, 288, S420), (250, 130), RS.CUBIC, lambda fmt: nv12(fmt, dict(pad=(5, 3, 7), stride_pad=37), 10)),
    "yuyv-422-of-444":  ((320, 240, S444), (321, 239), RS.CUBIC, yuyv422),
    "444-linear-of-420": ((352, 288, S420), (176, 144), RS.CUBIC, planar444_linear),
    "444-linear-of-420-odd": ((352, 288, S420), (45, 37), RS.TENT, planar444_linear),
    "rgb24":            ((352, 288, S420), (176, 144), RS.CUBIC, rgb24),
    "rgb24-of-422":     ((360, 200, S422), (45, 25), RS.TENT, rgb24),
}


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("name", sorted(FORMATS))
def test_batched_decoder_with_a_format_on_top(pkg, orc, name, on_device):
    """scale-then-format in numpy: the format's chroma halving or doubling, depth, packing or RGB matrix at the scaled geometry"""
    (w, h, fmt), target, filt, out = FORMATS[name]
    _, packets, want = streams_of(w, h, fmt)
    st = dict(name=name, scale=target + (filt,), out=out(fmt))
    count = run_scaled(pkg, packets, lambda s, t: want[s][t], w, h, fmt, 4, lambda k: st, on_device)
    assert count == [len(x) for x in want]


@pytest.mark.parametrize("on_device", [False, True])
def test_setter_order_and_switching(pkg, orc, on_device):
    """a format set before the scale is dropped by it; scale on, another scale with a format, the same scale without, off: after "off"
    the bytes are exactly today's packed planar frames"""
    w, h, fmt = 352, 288, S420
    _, packets, want = streams_of(w, h, fmt)
    f = PF.pf(PF.SEMI_UV)

    def pre(pkg, d):                                     # NV12 of the geometry in force is set when the next scale arrives, which drops it
        dims = d.out_dims
        d.set_output_format(cpf(pkg, f), S420)
        assert d.frame_bytes == PF.frame_bytes(f, dims[0], dims[1], S420) and d.out_dims == dims

    plan = ([dict(name="a", scale=(176, 144, RS.CUBIC), pre=pre, out=planar(fmt))] * 2 + [dict(name="b", scale=(704, 576, RS.TENT), out=nv12(fmt))] * 2 +
            [dict(name="c", scale=(704, 576, RS.TENT), pre=pre, out=planar(fmt))] * 1 + [dict(name="off", scale=None, pre=pre, out=planar(fmt))] * 9)
    count = run_scaled(pkg, packets, lambda s, t: want[s][t], w, h, fmt, 4, lambda k: plan[k], on_device)
    assert count == [len(x) for x in want]


@pytest.mark.parametrize("on_device", [False, True])
def test_overlay_under_the_scale(pkg, on_device):
    """set_draw_info(7) plus a scale: the overlay is drawn at the stream's resolution, then scaled: resample(definition(plain decode))"""
    from _drawinfo_cases import FRAMES
    w, h, streams, pics, plain, drawn = decoder_case(pkg, "96x64", S420)
    assert (drawn != plain).any()
    for (dw, dh, filt) in [(63, 40, RS.CUBIC), (192, 128, RS.TENT)]:
        got = run_drawn(pkg, w, h, S420, pics, [7] * FRAMES, setting=lambda d: d.set_output_scale(dw, dh, filt), on_device=on_device)
        for k in range(FRAMES):
            for s in range(3):
                exp = scaled(("drawn", k, s), drawn[k, s], w, h, S420, dw, dh, filt)
                A.assert_same("call %d stream %d at %dx%d" % (k, s, dw, dh), got[k, s], exp)
        undrawn = np.stack([RS.resample_frame(plain[k, 0], w, h, S420, dw, dh, filt) for k in range(FRAMES)])
        assert (undrawn != got[:, 0]).any(), "the overlay does not show in the scaled frames"


def test_escape_redo_keeps_the_scale_and_the_format(pkg, orc):
    """tests/test_gpu_pixout.py test_escape_redo_keeps_the_format with a scale in force: the second pass writes the scaled NV12 frame
    again, and the redo counter rises by one for that call only"""
    w, h, fmt, S = 352, 288, S444, 4
    dw, dh, filt = 176, 144, RS.CUBIC
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
    f = PF.pf(PF.SEMI_UV)
    d = pkg.DecBatch(w, h, fmt, S)
    try:
        d.set_output_scale(dw, dh, filt)
        d.set_output_format(cpf(pkg, f), S420)
        assert d.frame_bytes == PF.frame_bytes(f, dw, dh, S420)
        k = 0
        for p in pk:
            before = L.dsvg_ctx_decoder_redone(d.ctx)
            _, status, fnum = d.decode([p] * S, on_device=True)
            if status[0] == 0 and (p[5] & 4):
                frames = d.download()                    # (synchronises: the flags are settled here)
                exp = PO.export(RS.resample_frame(want[k], w, h, fmt, dw, dh, filt)[None], f, dw, dh, fmt, S420, 1)
                for s in range(S):
                    assert np.array_equal(frames[s], exp), "picture %d stream %d: first difference at %s" % (k, s, np.argwhere(frames[s] != exp)[:3].ravel())
                assert L.dsvg_ctx_decoder_redone(d.ctx) - before == (1 if k == 1 else 0)
                k += 1
        assert k == 2
    finally:
        d.close()


def test_refusals(pkg, orc):
    w, h, fmt = 352, 288, S420
    L = pkg.lib()
    _, packets, want = streams_of(w, h, fmt)
    dw, dh, filt = 176, 144, RS.CUBIC
    f = PF.pf(PF.SEMI_UV)
    fb_planar, fb_nv12 = A.frame_bytes(dw, dh, fmt), PF.frame_bytes(f, dw, dh, S420)
    status, fnum = (C.c_int * 1)(), (C.c_uint32 * 1)()
    pics = [p for p in packets[0] if p[5] & 4]
    state = dict(t=0)

    def decode_next(d, expected_of, fb):
        """the setting in force still decodes correctly: the next picture, into a buffer of its own"""
        p = pics[state["t"]]
        buf = (pkg.Buf * 1)()
        keep = np.frombuffer(bytes(p) + b"\0" * 16, dtype=np.uint8).copy()
        buf[0].data, buf[0].len = keep.ctypes.data_as(C.POINTER(C.c_uint8)), len(p)
        out = np.full((1, fb), 0x5A, dtype=np.uint8)
        held = out.copy()
        assert L.dsv1_decbatch_decode(d.h, buf, out.ctypes.data, fb - 1, 0, status, fnum) == DSVG_ERR_ARG     # an out_pitch below the scaled frame
        assert np.array_equal(out, held)
        assert L.dsv1_decbatch_decode(d.h, buf, out.ctypes.data, 0, 0, status, fnum) == 0 and status[0] == 0
        x = scaled(("dec", 0, state["t"]), want[0][state["t"]], w, h, fmt, dw, dh, filt)
        assert np.array_equal(out[0], expected_of(x)), "picture %d" % state["t"]
        state["t"] += 1

    d = pkg.DecBatch(w, h, fmt, 1)
    try:
        d.set_output_scale(dw, dh, filt)
        bad_scales = [t + (RS.CUBIC,) for g, ts in sorted(OC.REFUSED.items()) if g == (w, h, fmt) for t in ts] + [(dw, dh, 2), (dw, dh, -1), (dw, 0, filt)]
        assert (43, 36, RS.CUBIC) in bad_scales and (2817, 288, RS.CUBIC) in bad_scales
        for bad in bad_scales:
            assert L.dsv1_decbatch_set_output_scale(d.h, *bad) == DSVG_ERR_ARG, bad
            with pytest.raises(ValueError):
                d.set_output_scale(*bad)
            assert d.out_dims == (dw, dh) and d.frame_bytes == fb_planar == L.dsv1_decbatch_out_frame_bytes(d.h)
        decode_next(d, lambda x: x, fb_planar)
        # a format on top; then refused scales and refused formats leave scale AND format in force
        d.set_output_format(cpf(pkg, f), S420)
        assert d.frame_bytes == fb_nv12
        for bad in bad_scales[:3]:
            with pytest.raises(ValueError):
                d.set_output_scale(*bad)
            assert d.out_dims == (dw, dh) and d.frame_bytes == fb_nv12 == L.dsv1_decbatch_out_frame_bytes(d.h)
        # explicit pitches that fit the stream's geometry but are asked for the scaled one: dw - 1 is too small for a dw-wide row; the
        # frame stride of the scaled NV12 frame less one; the full-size frame's own pitch is fine
        for badf in [PF.pf(PF.SEMI_UV, pitch=(dw - 1, 0, 0)), PF.pf(PF.SEMI_UV, pitch=(dw, dw - 1, 0)), PF.pf(PF.SEMI_UV, frame_bytes=fb_nv12 - 1)]:
            assert L.dsv1_decbatch_set_output_format(d.h, C.byref(cpf(pkg, badf)), S420) == DSVG_ERR_ARG, badf
            with pytest.raises(ValueError):
                d.set_output_format(cpf(pkg, badf), S420)
            assert d.frame_bytes == fb_nv12 and d.out_dims == (dw, dh)
        decode_next(d, lambda x: PO.export(x[None], f, dw, dh, fmt, S420, 1), fb_nv12)
        wide = PF.pf(PF.SEMI_UV, pitch=(w, w, 0))            # the stream's own pitches hold a scaled row
        d.set_output_format(cpf(pkg, wide), S420)
        decode_next(d, lambda x: PO.export(x[None], wide, dw, dh, fmt, S420, 1, into=np.full(PF.frame_bytes(wide, dw, dh, S420), 0x5A, np.uint8)),
                    PF.frame_bytes(wide, dw, dh, S420))
        for edge in OC.ACCEPTED_EDGE[(w, h, fmt)]:           # the allowed side of the bound is taken
            d.set_output_scale(*edge)
            assert d.out_dims == edge
        assert state["t"] >= 3
    finally:
        d.close()
    assert not d.h                                       # closed: the handle is gone, and a NULL handle is refused
    assert L.dsv1_decbatch_set_output_scale(d.h, dw, dh, filt) == DSVG_ERR_ARG
    assert L.dsv1_decbatch_set_output_scale(None, 0, 0, filt) == DSVG_ERR_ARG
    with pytest.raises(ValueError):
        d.set_output_scale(dw, dh)
