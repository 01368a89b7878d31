"""The decoders' debug overlay on the GPU (include/dsv1_api.h, debug overlays; csrc/k_drawinfo.hip): dsv1_draw_info_clip equals the
sequential definition tests/_drawinfo.py byte for byte on synthetic tables in which the writers collide both ways round; the batched
decoder with an overlay set writes export(definition(plain decode)) in every output setting, leaves its references clean and matches
the reference CLI's -drawinfo7 hashes of tests/golden/drawinfo.json; the drop-in dsv_dec and the reference's CLI on this library
write what the reference writes."""
import ctypes as C
import hashlib
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _cabi as A
import _drawinfo as DI
import _drawinfo_cases as K
import _pixfmt as PF
import blocksize_cases as BC
from test_gpu_denoise import DevMem

pytestmark = pytest.mark.gpu

S444, S422, S420, S411 = A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411
DROPIN = os.path.join(A.ROOT, "oracle", "_ref", "dsv1_dropin")


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


def cpf(pkg, f):
    return pkg.PixFormat(f["layout"], f["depth"], f["msb"], f["pitch"], f["frame_bytes"])


# ---- 1. the kernel against the definition --------------------------------------------------------------------------------------
KERNEL_CASES = [(g, S420) for g in K.KERNEL_GEOMS] + [(K.KERNEL_GEOMS[0], f) for f in (S444, S422, S411)]


@pytest.mark.parametrize("geom,fmt", KERNEL_CASES, ids=["%dx%d-%dx%d-0x%x" % (g + (f,)) for g, f in KERNEL_CASES])
def test_draw_info_clip_equals_the_definition(pkg, mem, geom, fmt):
    w, h, bw, bh = geom
    tabs = K.kernel_tables(w, h, bw, bh)
    n, fb = tabs.shape[0], A.frame_bytes(w, h, fmt)
    clip = np.random.default_rng(w * h + fmt).integers(1, 255, (n, fb), dtype=np.uint8)       # (neither 0 nor 255: every mark shows)
    for mode in range(1, 8):
        traces = [{} for _ in range(n)]
        want = DI.draw_frames(clip, w, h, bw, bh, tabs, mode, traces)
        if mode == 7:
            seen = set().union(*traces)
            assert not [c for c in K.CONFLICTS if c not in seen], "the tables do not make these writers meet"
            assert w % bw == 0 or any("dots_clipped" in t for t in traces), "no dot of an edge block falls outside the plane"
            assert (want[:, :w * h] == 255).any() and (want != clip).any()
        A.assert_same("chroma in the definition", want[:, w * h:], clip[:, w * h:])
        got = pkg.draw_info_clip(clip, w, h, fmt, bw, bh, tabs, mode)
        for t in range(n):
            A.assert_same("host clip, mode %d, picture %d" % (mode, t), got[t, :w * h], want[t, :w * h], shape=(h, w))
        A.assert_same("host clip, mode %d, chroma" % mode, got[:, w * h:], clip[:, w * h:])
        guard = 256                                      # device clip, with the bytes around it
        buf = np.concatenate([np.full(guard, 0x5A, np.uint8), clip.reshape(-1), np.full(guard, 0xA5, np.uint8)])
        d = mem.alloc(buf)
        pkg.draw_info_clip(C.c_void_p(d.value + guard), w, h, fmt, bw, bh, tabs, mode, n=n)
        back = mem.read(d, buf.size)
        assert (back[:guard] == 0x5A).all() and (back[-guard:] == 0xA5).all()
        A.assert_same("device clip, mode %d" % mode, back[guard:-guard].reshape(n, fb), want)


def test_draw_info_clip_refusals(pkg):
    w, h, n = 96, 64, 3
    clip = np.zeros((n, A.frame_bytes(w, h, S444)), dtype=np.uint8)
    tab = np.zeros(n * 12 * 8, dtype=DI.BLOCKINFO)      # (room for blocks of 8 x 8, were they taken)
    L = pkg.lib()
    ok = dict(fmt=S420, blk_w=16, blk_h=16, mode=7)
    for bad in (dict(mode=0), dict(mode=8), dict(mode=-1), dict(blk_w=8), dict(blk_w=72), dict(blk_h=8), dict(blk_h=72), dict(fmt=0x3), dict(fmt=0x15)):
        kw = dict(ok, **bad)
        assert L.dsv1_draw_info_clip(0, clip.ctypes.data, w, h, kw["fmt"], n, kw["blk_w"], kw["blk_h"], tab.ctypes.data, kw["mode"], 0) == -2, bad
    assert L.dsv1_draw_info_clip(0, None, w, h, S420, n, 16, 16, tab.ctypes.data, 7, 0) == -2
    assert L.dsv1_draw_info_clip(0, clip.ctypes.data, w, h, S420, n, 16, 16, None, 7, 0) == -2
    for kw in (dict(blk_w=16, blk_h=16, mode=8), dict(blk_w=8, blk_h=16, mode=7), dict(blk_w=16, blk_h=72, mode=1)):
        with pytest.raises(ValueError):
            pkg.draw_info_clip(clip[:, :A.frame_bytes(w, h, S420)], w, h, S420, info=tab, **kw)
    assert not clip.any()


# ---- 2. the batched decoder ----------------------------------------------------------------------------------------------------
_cases = {}


def decoder_case(pkg, name, fmt):
    """three streams of one fixture geometry -- the fixture's own, an I-only one, a third clip -- with their picture packets, the plain
    decode of this library and the definition applied to it at mode 7; made once"""
    if (name, fmt) not in _cases:
        w, h, seed = K.STREAMS[name]
        clip = K.stream_clip(name, fmt)
        other = A.gen_clip(w, h, fmt, seed + 0x100, K.FRAMES, style=1)
        streams = [bytes(pkg.encode_clip(clip, w, h, fmt, **K.KW)), bytes(pkg.encode_clip(clip, w, h, fmt, qp=85, gop=0, rc_mode_cli=1)),
                   bytes(pkg.encode_clip(other, w, h, fmt, **K.KW))]
        pics = [K.picture_packets(s) for s in streams]
        assert all(len(p) == K.FRAMES for p in pics) and not any(p[5] & 1 for p in pics[1])
        plain = run(pkg, w, h, fmt, pics, [0] * K.FRAMES)
        want = np.stack([K.define(pkg, streams[s], plain[:, s], w, h, 7) for s in range(3)], axis=1)
        _cases[(name, fmt)] = (w, h, streams, pics, plain, want)
    return _cases[(name, fmt)]


def run(pkg, w, h, fmt, pics, modes, setting=None, on_device=False, before_close=None):
    """the batch over the calls with modes[k] in force: [calls][streams][frame bytes]; before_close(d): called after the last call"""
    d = pkg.DecBatch(w, h, fmt, len(pics))
    try:
        if setting:
            setting(d)
        out, cur = [], None
        for k, mode in enumerate(modes):
            if mode != cur:
                d.set_draw_info(mode)
                cur = mode
            pk = [p[k] for p in pics]
            if on_device:
                _, status, fnum = d.decode(pk, on_device=True)
                frames = d.download()
            else:
                frames, status, fnum = d.decode(pk)
            assert list(status) == [0] * len(pics) and list(fnum) == [k] * len(pics)
            out.append(np.array(frames, copy=True))
        if before_close:
            before_close(d)
        return np.stack(out)
    finally:
        d.close()


DECODER_CASES = [("96x64", S420), ("352x288", S420), ("96x64", S444)]


@pytest.mark.parametrize("name,fmt", DECODER_CASES)
def test_batched_decoder_packed_planar(pkg, name, fmt):
    w, h, streams, pics, plain, want = decoder_case(pkg, name, fmt)
    nP = sum(1 for p in pics[0] if p[5] & 1)
    assert nP >= 3 and (want[:, 0] != plain[:, 0]).any()
    for on_device in (False, True):
        got = run(pkg, w, h, fmt, pics, [7] * K.FRAMES, on_device=on_device)
        for k in range(K.FRAMES):
            for s in range(3):
                A.assert_same("call %d stream %d luma (device %d)" % (k, s, on_device), got[k, s, :w * h], want[k, s, :w * h], shape=(h, w))
                A.assert_same("call %d stream %d chroma" % (k, s), got[k, s, w * h:], plain[k, s, w * h:])
                if not pics[s][k][5] & 1:
                    A.assert_same("I picture %d of stream %d" % (k, s), got[k, s], plain[k, s])
        A.assert_same("the I-only stream", got[:, 1], plain[:, 1])
        if fmt == S420:
            assert hashlib.sha256(got[:, 0].tobytes()).hexdigest() == K.goldens()[name], "not the reference CLI's -drawinfo7 output"
    if fmt == S420:                                      # the fixture is the reference CLI's stream, and the plain decode the reference's
        assert hashlib.sha256(want[:, 0].tobytes()).hexdigest() == K.goldens()[name]


@pytest.mark.parametrize("name,fmt", DECODER_CASES)
def test_batched_decoder_switching_the_mode(pkg, name, fmt):
    w, h, streams, pics, plain, want = decoder_case(pkg, name, fmt)
    modes = [7, 7, 0, 0, 7, 7]
    for on_device in (False, True):
        got = run(pkg, w, h, fmt, pics, modes, on_device=on_device)
        for k, m in enumerate(modes):
            A.assert_same("call %d, mode %d (device %d)" % (k, m, on_device), got[k], want[k] if m else plain[k])
    got = run(pkg, w, h, fmt, pics, [2, 5, 1, 4, 3, 6])
    for k, m in enumerate([2, 5, 1, 4, 3, 6]):
        for s in range(3):
            A.assert_same("call %d, mode %d, stream %d" % (k, m, s), got[k, s], K.define(pkg, streams[s], plain[:, s], w, h, m)[k])


@pytest.mark.parametrize("name,fmt", DECODER_CASES)
@pytest.mark.parametrize("out", ["nv12", "uyvy-422-linear", "rgb24-bt709"])
def test_batched_decoder_output_formats(pkg, name, fmt, out):
    """the overlay is on the decoded luma BEFORE the one output pass: a frame is export(definition(plain decode))"""
    w, h, streams, pics, plain, want = decoder_case(pkg, name, fmt)
    flat = want.reshape(K.FRAMES * 3, -1)
    if out == "nv12":
        osub = S420                                      # (the 4:4:4 streams: chroma halved both ways in the same pass)
        exp = pkg.export_clip(flat, w, h, fmt, cpf(pkg, PF.pf(PF.SEMI_UV)), osub)
        setting = lambda d: d.set_output_format(cpf(pkg, PF.pf(PF.SEMI_UV)), osub)                              # noqa: E731
    elif out == "uyvy-422-linear":
        exp = pkg.export_clip(flat, w, h, fmt, cpf(pkg, PF.pf(PF.UYVY)), S422, upsample=pkg.CHROMA_LINEAR)
        setting = lambda d: d.set_output_format(cpf(pkg, PF.pf(PF.UYVY)), S422, upsample=pkg.CHROMA_LINEAR)     # noqa: E731
    else:
        rf = pkg.RgbFormat(pkg.RGB_RGB24, pkg.MATRIX_BT709)
        exp = pkg.rgb_export_clip(flat, w, h, fmt, rf)
        setting = lambda d: d.set_output_rgb(rf)                                                               # noqa: E731
    exp = exp.reshape(K.FRAMES, 3, -1)
    for on_device in (False, True):
        got = run(pkg, w, h, fmt, pics, [7] * K.FRAMES, setting=setting, on_device=on_device)
        A.assert_same("%s (device %d)" % (out, on_device), got, exp)


def test_mode_refusals_and_a_rebuilt_context(pkg, orc):
    """streams whose block size is not the rule's (tests/blocksize_cases.py): the batch builds a new context at their first picture,
    after the overlay was set"""
    w, h, fmt, n, stream = BC.make_stream(0)
    assert tuple(A.block_dims(w, h)[:2]) != (32, 24)
    plain = np.stack(A.orc_decode(stream, w, h, fmt))
    want = K.define(pkg, stream, plain, w, h, 7)
    assert pkg.packet_blockinfo(K.picture_packets(stream)[1], w, h)[:2] == (32, 24) and (want != plain).any()
    d = pkg.DecBatch(w, h, fmt, 2)
    try:
        for bad in (-1, 8, 255):
            with pytest.raises(ValueError):
                d.set_draw_info(bad)
        d.set_draw_info(7)
        for t, p in enumerate(K.picture_packets(stream)):
            out, status, fnum = d.decode([p] * 2)
            assert list(status) == [0, 0]
            A.assert_same("picture %d" % t, out[0], want[t])
            A.assert_same("picture %d, second stream" % t, out[1], want[t])
    finally:
        d.close()
    assert pkg.lib().dsv1_decbatch_set_draw_info(None, 7) == -2


# ---- 3. the drop-in ------------------------------------------------------------------------------------------------------------
class Decoder(C.Structure):
    _fields_ = [("vidmeta", A.Meta), ("ref", C.c_void_p), ("draw_info", C.c_int), ("got_metadata", C.c_int)]


def lib_decode(L, stream, draw_info, last_error=None):
    """dsv_dec of library L (this one, or the compiled reference: the same structs), packet by packet: decoded frames, packed planar"""
    L.dsv_alloc.restype = C.c_void_p
    L.dsv_alloc.argtypes = [C.c_int]
    L.dsv_dec.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
    L.dsv_frame_ref_dec.argtypes = [C.c_void_p]
    L.dsv_dec_free.argtypes = [C.c_void_p]
    dec = Decoder()
    dec.draw_info = draw_info
    got = []
    try:
        for p in A.split_packets(stream):
            buf = A.Buf()
            m = L.dsv_alloc(len(p))
            C.memmove(m, p, len(p))
            buf.data = C.cast(m, C.POINTER(C.c_uint8))
            buf.len = len(p)
            frame = C.c_void_p(None)
            fn = C.c_uint32(0)
            rc = L.dsv_dec(C.byref(dec), C.byref(buf), C.byref(frame), C.byref(fn))
            assert rc != 1, "dsv_dec error"
            if rc == 0 and frame.value:
                f = C.cast(frame, C.POINTER(A.Frame)).contents
                planes = []
                for c in range(3):
                    pl = f.planes[c]
                    arr = np.ctypeslib.as_array(pl.data, shape=(pl.h * pl.stride,))
                    planes.append(np.lib.stride_tricks.as_strided(arr, shape=(pl.h, pl.w), strides=(pl.stride, 1)).copy().reshape(-1))
                got.append(np.concatenate(planes))
                L.dsv_frame_ref_dec(frame)
    finally:
        L.dsv_dec_free(C.byref(dec))
    return got


@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("name", ["96x64", "384x240"])
def test_drop_in_dsv_dec_equals_the_reference_library(pkg, ref, monkeypatch, name, pool):
    """both ways a frame comes back: the pinned frame pool, and the packed download (DSV1_DEC_NO_POOL)"""
    if not pool:
        monkeypatch.setenv("DSV1_DEC_NO_POOL", "1")
    w, h, _ = K.STREAMS[name]
    stream = bytes(pkg.encode_clip(K.stream_clip(name), w, h, S420, **K.KW))
    for mode in (7, 2, 8):
        want = lib_decode(ref, stream, mode)
        got = lib_decode(pkg.lib(), stream, mode)
        assert len(got) == len(want) == K.FRAMES
        for t in range(K.FRAMES):
            A.assert_same("%s draw_info %d picture %d" % (name, mode, t), got[t], want[t])
        if mode == 7:
            assert hashlib.sha256(np.stack(got).tobytes()).hexdigest() == K.goldens()[name]
    assert any((a != b).any() for a, b in zip(lib_decode(pkg.lib(), stream, 8), lib_decode(pkg.lib(), stream, 0)))


def test_drop_in_dsv_dec_matches_the_golden_hashes(pkg):
    """needs no compiled reference"""
    for name in ("96x64", "384x240"):
        w, h, _ = K.STREAMS[name]
        stream = bytes(pkg.encode_clip(K.stream_clip(name), w, h, S420, **K.KW))
        got = lib_decode(pkg.lib(), stream, 7)
        assert hashlib.sha256(np.stack(got).tobytes()).hexdigest() == K.goldens()[name], name


def test_reference_cli_on_this_library_drawinfo():
    if not (os.path.exists(DROPIN) and os.path.exists(A.REF_CLI)):
        pytest.skip("oracle/_ref binaries were not built")
    w, h, n = 352, 288, 9
    clip = K.stream_clip("352x288", frames=n)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = A.PKG_DIR + ":" + env.get("LD_LIBRARY_PATH", "")
    with tempfile.TemporaryDirectory() as td:
        A.ref_cli_encode(clip, w, h, A.FMT_CLI[S420], K.CLI, td)
        outs = []
        for binary, e in ((A.REF_CLI, None), (DROPIN, env)):
            yuv = os.path.join(td, os.path.basename(binary) + ".yuv")
            r = subprocess.run([binary, "d", "-y", "-inp_" + os.path.join(td, "out.dsv"), "-out_" + yuv, "-drawinfo7"], stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, env=e, timeout=300)
            assert r.returncode == 0, r.stdout.decode(errors="replace")[-400:]
            outs.append(np.fromfile(yuv, dtype=np.uint8))
        plain = os.path.join(td, "plain.yuv")
        subprocess.run([A.REF_CLI, "d", "-y", "-inp_" + os.path.join(td, "out.dsv"), "-out_" + plain], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        assert (np.fromfile(plain, dtype=np.uint8) != outs[0]).any()
        A.assert_same("dsv1_dropin d -drawinfo7", outs[1], outs[0])
