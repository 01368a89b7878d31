"""Decoder output formats on the GPU (include/dsv1_api.h, csrc/k_pixout.hip): dsv1_export_clip equals the numpy statement
tests/_pixout.py byte for byte over every valid format and every allowed pair of subsamplings, on the 16-byte path and on the byte
path, leaving padding and surroundings as they were; converting what it wrote gives the frames back; the batched decoder writes NV12 /
P010 / YUYV / UYVY / 10-bit planar frames of the oracle's pictures, halving chroma on the way, with host and device output, through
the int32 second pass too."""
import ctypes as C
import importlib
import itertools
import os
import subprocess

import numpy as np
import pytest

import _cabi as A
import _pixfmt as PF
import _pixout as PO
from test_gpu_pixfmt import DevMem, padded
from test_gpu_decode_escape import _two_picture_stream, plane_payload, region_base, splice

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2
GUARD = 256


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return m


@pytest.fixture
def mem(pkg):
    m = DevMem(pkg)                                      # (per test: what a geometry's cases allocated goes with it)
    yield m
    m.close()


def cpf(pkg, f):
    return pkg.PixFormat(f["layout"], f["depth"], f["msb"], f["pitch"], f["frame_bytes"])


def formats():
    for layout, depth, msb in itertools.product(PF.LAYOUTS, PF.DEPTHS, (0, 1)):
        if depth > 8 or not msb:
            yield PF.pf(layout, depth, msb)


def valid_cases(w, h):
    """(format, stream subsampling, output subsampling): every valid format at every allowed pair"""
    for fmt, ofmt in itertools.product(PF.SUBSAMPS, PF.SUBSAMPS):
        for f in formats():
            if PO.valid(f, w, h, fmt, ofmt):
                yield f, fmt, ofmt


def segments_fast(f, w, h, fmt, ofmt):
    """per output plane: does every row start 16-byte aligned, inputs (tightly packed planar frames) and output (8 for the U and V a
    packed layout takes as they are), with buffers that start aligned -- the kernel's rule for its 16-byte path (csrc/k_pixout.hip:
    po_seg_fast)"""
    lay, _, fb = PF.plane_layout(f, w, h, ofmt)
    cw, ch = A.chroma_dims(w, h, fmt)
    sfb = A.frame_bytes(w, h, fmt)
    Y, U, V = (0, w, 16), (w * h, cw, 16), (w * h + cw * ch, cw, 16)
    if f["layout"] in (PF.YUYV, PF.UYVY) and A.hshift(fmt) == A.hshift(ofmt):
        U, V = U[:2] + (8,), V[:2] + (8,)
    ins = {PF.PLANAR: [[Y], [U], [V]], PF.SEMI_UV: [[Y], [U, V]], PF.YUYV: [[Y, U, V]]}
    ins[PF.SEMI_VU], ins[PF.UYVY] = ins[PF.SEMI_UV], ins[PF.YUYV]
    return [(fb | off | pitch) % 16 == 0 and all((sfb | ioff | ip) % al == 0 for ioff, ip, al in i)
            for (off, pitch, _, _), i in zip(lay, ins[f["layout"]])]


# 352x288: every row on the 16-byte path; 250x130: none aligned; 36x20: chroma rows of one tail, or one step plus a tail; 35x19: odd --
# both clamps of the halving and the odd packed row; 48x18: aligned rows that end in a tail (24 chroma pairs of a halved 4:4:4 row)
GEOMS = [(352, 288), (250, 130), (36, 20), (35, 19), (1, 1), (48, 18)]
PADS = [None, dict(pad=(48, 16, 80), stride_pad=256), dict(pad=(5, 3, 7), stride_pad=37)]


def test_geometry_list_reaches_the_vector_path_the_byte_path_and_mixed_segments():
    """from the geometry alone"""
    S420, S422, S444, S411 = A.SUBSAMP_420, A.SUBSAMP_422, A.SUBSAMP_444, A.SUBSAMP_411
    nv12, p010 = PF.pf(PF.SEMI_UV), PF.pf(PF.SEMI_UV, 10, 1)
    assert (352, 288) in GEOMS and (250, 130) in GEOMS and (36, 20) in GEOMS and (35, 19) in GEOMS and (48, 18) in GEOMS
    for f in (nv12, p010, PF.pf(PF.PLANAR, 10, 0)):
        for fmt in (S420, S422, S444):                   # as they are, and halved horizontally, vertically, both ways
            assert all(segments_fast(f, 352, 288, fmt, S420))
            assert all(segments_fast(padded(f, 352, 288, S420, **PADS[1]), 352, 288, fmt, S420))
            assert not any(segments_fast(f, 250, 130, fmt, S420))
            assert not any(segments_fast(padded(f, 352, 288, S420, **PADS[2]), 352, 288, fmt, S420))
    for fmt in (S422, S444):
        assert all(segments_fast(PF.pf(PF.YUYV), 352, 288, fmt, S422)) and not any(segments_fast(PF.pf(PF.UYVY), 250, 130, fmt, S422))
    assert segments_fast(PF.pf(PF.PLANAR), 352, 288, S411, S411) == [True, False, False]          # mixed: 88-byte chroma rows
    assert segments_fast(PF.pf(PF.PLANAR), 352, 288, S444, S420) == [True, True, True]
    assert A.chroma_dims(36, 20, S411)[0] < 16 and 36 // 2 == 18          # (36x20: chroma rows of one tail, or one step + a tail)
    # 48x18, 4:4:4 -> 4:2:0 NV12: every row aligned, and the 24 pairs of a chroma row are one whole step and a tail of 8
    assert segments_fast(nv12, 48, 18, S444, S420) == [True, True] and A.chroma_dims(48, 18, S420)[0] == 24
    # 35x19: odd chroma planes at 4:4:4 and 4:2:2 (the repeated last column / row), and an odd packed row
    assert A.chroma_dims(35, 19, S444) == (35, 19) and A.chroma_dims(35, 19, S422) == (18, 19) and 35 % 2 == 1


@pytest.mark.parametrize("w,h", GEOMS)
def test_export_clip_equals_numpy(pkg, mem, w, h):
    """whole destination compared, 256 guard bytes before and after included: padding and surroundings are as they were"""
    n, ncases = 3, 0
    for i, (f0, fmt, ofmt) in enumerate(valid_cases(w, h)):
        rng = np.random.default_rng(7000 + i)
        x = rng.integers(0, 256, (n, A.frame_bytes(w, h, fmt)), dtype=np.uint8)
        x[:, :2], x[:, -2:] = 255, 255                   # (255 + 255 + 1 must keep its carry)
        src_d = mem.alloc(x)
        for pad in PADS:
            f = f0 if pad is None else padded(f0, w, h, ofmt, **pad)
            fb = PF.frame_bytes(f, w, h, ofmt)
            before = rng.integers(0, 256, GUARD + n * fb + GUARD, dtype=np.uint8)
            want = before.copy()
            PO.export(x, f, w, h, fmt, ofmt, n, into=want[GUARD:GUARD + n * fb])
            what = "%s 0x%x -> 0x%x %dx%d" % (f, fmt, ofmt, w, h)
            got = before.copy()
            pkg.export_clip(x, w, h, fmt, cpf(pkg, f), ofmt, out=got[GUARD:GUARD + n * fb])
            assert np.array_equal(got, want), "host %s: first difference at %s" % (what, np.argwhere(got != want)[:3].ravel())
            dst_d = mem.alloc(before)
            pkg.export_clip(src_d, w, h, fmt, cpf(pkg, f), ofmt, n=n, out=C.c_void_p(dst_d.value + GUARD))
            got = mem.read(dst_d, before.size)
            assert np.array_equal(got, want), "device %s: first difference at %s" % (what, np.argwhere(got != want)[:3].ravel())
            ncases += 1
    assert ncases >= 3 * 100


@pytest.mark.parametrize("w,h", [(352, 288), (250, 130)])
@pytest.mark.parametrize("name", ["nv12", "p010", "yuyv", "yuv420p12"])
def test_round_trip_on_the_device(pkg, name, w, h):
    f, fmt = {"nv12": (PF.pf(PF.SEMI_UV), A.SUBSAMP_420), "p010": (PF.pf(PF.SEMI_UV, 10, 1), A.SUBSAMP_420),
              "yuyv": (PF.pf(PF.YUYV), A.SUBSAMP_422), "yuv420p12": (PF.pf(PF.PLANAR, 12, 0), A.SUBSAMP_420)}[name]
    x = np.random.default_rng(w + len(name)).integers(0, 256, (3, A.frame_bytes(w, h, fmt)), dtype=np.uint8)
    for g in (f, padded(f, w, h, fmt)):
        raw = pkg.export_clip(x, w, h, fmt, cpf(pkg, g))
        assert raw.shape == (3, PF.frame_bytes(g, w, h, fmt))
        assert np.array_equal(pkg.convert_clip(raw, cpf(pkg, g), w, h, fmt), x), g


# ---- batched decoder ------------------------------------------------------------------------------------------------------------
_streams = {}


def streams_of(w, h, fmt):
    """as test_batched_decoder_matches_oracle: 4 streams, mixed GOP lengths, stream 3 intra-only, EOS at different calls; built once"""
    if (w, h, fmt) not in _streams:
        gops, nfr = [3, 5, 4, 0], [7, 9, 6, 4]
        data, packets, want = [], [], []
        for s in range(4):
            clip = A.gen_clip(w, h, fmt, 0xDEC0 + 16 * s + w, nfr[s], style=s % 3)
            st, _ = A.orc_encode(clip, A.orc_cfg(w, h, fmt, qp=85 if s != 1 else 60, gop=gops[s], rc_mode_cli=1))
            data.append(st)
            packets.append(A.split_packets(st))
            want.append(A.orc_decode(st, w, h, fmt))
            assert len(want[s]) == nfr[s]
        _streams[(w, h, fmt)] = (data, packets, want)
    return _streams[(w, h, fmt)]


OUTPUTS = {
    "420-nv12":        (352, 288, A.SUBSAMP_420, PF.pf(PF.SEMI_UV), A.SUBSAMP_420, None),
    "420-p010-padded": (352, 288, A.SUBSAMP_420, PF.pf(PF.SEMI_UV, 10, 1), A.SUBSAMP_420, dict(pad=(48, 16, 80), stride_pad=256)),
    "444-nv12-420":    (320, 240, A.SUBSAMP_444, PF.pf(PF.SEMI_UV), A.SUBSAMP_420, None),
    "444-yuyv-422":    (320, 240, A.SUBSAMP_444, PF.pf(PF.YUYV), A.SUBSAMP_422, None),
    "444-planar10msb": (320, 240, A.SUBSAMP_444, PF.pf(PF.PLANAR, 10, 1), A.SUBSAMP_444, None),
    "422-uyvy":        (360, 200, A.SUBSAMP_422, PF.pf(PF.UYVY), A.SUBSAMP_422, None),
    "422-nv21-420":    (360, 200, A.SUBSAMP_422, PF.pf(PF.SEMI_VU), A.SUBSAMP_420, None),
}


def run_decoder(pkg, packets, w, h, fmt, S, setting, on_device, frame, seed=3):
    """decode the streams call by call with `setting(call)` -> (format dict or None, output subsampling) in force; after every call
    the WHOLE output buffer is compared with a host copy into which frame(s, k, format, ofmt, into) wrote the expected bytes of the
    streams that had a picture -- the other streams' frames, and every padding byte, keep the sentinel"""
    d = pkg.DecBatch(w, h, fmt, S)
    try:
        eos = bytes(packets[0][-1])
        count = [0] * S
        cur, expect, dev = "unset", None, None
        for k in range(max(len(p) for p in packets)):
            f, ofmt = setting(k)
            if (f, ofmt) != cur:
                d.set_output_format(None if f is None else cpf(pkg, f), ofmt)
                cur = (f, ofmt)
                fb = PF.frame_bytes(f or PF.pf(), w, h, ofmt)
                assert d.frame_bytes == fb == pkg.lib().dsv1_decbatch_out_frame_bytes(d.h)
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
                    frame(s, count[s], f, ofmt, expect[s * fb:(s + 1) * fb])
                    count[s] += 1
                else:
                    assert status[s] in (2, 3)
            assert np.array_equal(got, expect), "call %d: first difference at byte %s of %d-byte frames" % (k, np.argwhere(got != expect)[:3].ravel(), fb)
        return count
    finally:
        d.close()


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("name", sorted(OUTPUTS))
def test_batched_decoder_writes_the_format(pkg, orc, name, on_device):
    w, h, fmt, f, ofmt, pad = OUTPUTS[name]
    if pad:
        f = padded(f, w, h, ofmt, **pad)
    _, packets, want = streams_of(w, h, fmt)

    def frame(s, t, g, o, into):
        PO.export(want[s][t][None], g, w, h, fmt, o, 1, into=into)

    count = run_decoder(pkg, packets, w, h, fmt, 4, lambda k: (f, ofmt), on_device, frame)
    assert count == [len(x) for x in want]


@pytest.mark.parametrize("on_device", [False, True])
def test_switching_the_format_between_calls_and_back(pkg, orc, on_device):
    """NV12, then 4:2:2 YUYV, then NULL: today's packed planar bytes; then planar / 8 bits / tight, which is the default too"""
    w, h, fmt = 320, 240, A.SUBSAMP_444
    _, packets, want = streams_of(w, h, fmt)
    plan = [(PF.pf(PF.SEMI_UV), A.SUBSAMP_420)] * 3 + [(PF.pf(PF.YUYV), A.SUBSAMP_422)] * 2 + [(None, fmt)] * 3 + [(PF.pf(), fmt)] * 9

    def frame(s, t, g, o, into):
        if g is None or g == PF.pf():
            into[:] = want[s][t]
        else:
            PO.export(want[s][t][None], g, w, h, fmt, o, 1, into=into)

    run_decoder(pkg, packets, w, h, fmt, 4, lambda k: plan[k], on_device, frame)


@pytest.mark.parametrize("w,h,fmt", [(320, 240, A.SUBSAMP_444), (360, 200, A.SUBSAMP_422)])
def test_planar_420_output_equals_the_reference_cli_out420p(pkg, orc, ref, tmp_path, w, h, fmt):
    data, packets, want = streams_of(w, h, fmt)
    cli = []
    for s in (0, 3):
        inp, outp = str(tmp_path / ("s%d.dsv" % s)), str(tmp_path / ("s%d.yuv" % s))
        with open(inp, "wb") as fh:
            fh.write(data[s])
        subprocess.run([A.REF_CLI, "d", "-y", "-inp_" + inp, "-out_" + outp, "-out420p1"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        cli.append(np.fromfile(outp, dtype=np.uint8).reshape(len(want[s]), A.frame_bytes(w, h, A.SUBSAMP_420)))
        os.remove(outp)
    two = [packets[0], packets[3]]

    def frame(s, t, g, o, into):
        into[:] = cli[s][t]

    assert run_decoder(pkg, two, w, h, fmt, 2, lambda k: (PF.pf(), A.SUBSAMP_420), True, frame) == [len(cli[0]), len(cli[1])]


def test_escape_redo_keeps_the_format(pkg, orc):
    """a P picture with a symbol beyond int16 (tests/test_gpu_decode_escape.py) is decoded again from int32 coefficients after its
    NV12 frame was already written on the device: the second pass writes NV12 again, halved to 4:2:0, not a stale or a planar frame"""
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
    nv12 = PF.pf(PF.SEMI_UV)
    d = pkg.DecBatch(w, h, fmt, S)
    try:
        d.set_output_format(cpf(pkg, nv12), A.SUBSAMP_420)
        k = 0
        for p in pk:
            before = L.dsvg_ctx_decoder_redone(d.ctx)
            _, status, fnum = d.decode([p] * S, on_device=True)
            if status[0] == 0 and (p[5] & 4):
                frames = d.download()                    # (synchronises: the flags are settled here)
                exp = PO.export(want[k][None], nv12, w, h, fmt, A.SUBSAMP_420, 1)
                for s in range(S):
                    assert np.array_equal(frames[s], exp), "picture %d stream %d: first difference at %s" % (k, s, np.argwhere(frames[s] != exp)[:3].ravel())
                assert L.dsvg_ctx_decoder_redone(d.ctx) - before == (1 if k == 1 else 0)
                k += 1
        assert k == 2
    finally:
        d.close()


@pytest.mark.parametrize("setting", ["nv12-420", None])
def test_escape_redo_of_a_call_in_which_some_streams_have_no_picture(pkg, orc, setting):
    """the pass recorded with a call that is decoded again is replayed as it was asked for, also where only streams 0 and 2 of four
    had a picture: NV12 at 4:2:0 is one export with the frame indices {0, 2}; packed planar is one pass per picture, of which the
    second settles the call (the first is replayed behind the redo, the second still has to be written).  The frames of streams 1
    and 3 keep the sentinel, byte for byte"""
    w, h, fmt, S = 352, 288, A.SUBSAMP_444, 4
    pk, ip = _two_picture_stream(w, h, fmt, 0xE5CA9E)
    b2, sw2 = region_base(w, h, 2, 1)
    b1, sw1 = region_base(w, h, 1, 2)
    entries = sorted([(5, 3), (b1 + 4 * sw1 + 9, -2), (b2 + 10 * sw2 + 10, 40000), (b2 + 30 * sw2 + 77, 1)])
    pk[ip] = splice(pk[ip], {0: plane_payload(7, entries)})
    want = A.orc_decode(b"".join(pk), w, h, fmt)
    assert len(want) == 2
    eos = bytes(pk[-1])
    assert len(eos) == 14 and not (eos[5] & 4)
    ii = [i for i, p in enumerate(pk) if p[5] & 4][0]
    assert ii < ip
    L = pkg.lib()
    L.dsvg_ctx_decoder_redone.restype = C.c_long
    L.dsvg_ctx_decoder_redone.argtypes = [C.c_void_p]
    nv12 = PF.pf(PF.SEMI_UV)

    def expected(t):
        if setting is None:
            return want[t].reshape(-1)
        return PO.export(want[t][None], nv12, w, h, fmt, A.SUBSAMP_420, 1).reshape(-1)

    d = pkg.DecBatch(w, h, fmt, S)
    try:
        if setting is not None:
            d.set_output_format(cpf(pkg, nv12), A.SUBSAMP_420)
        dev = d.dev_alloc()
        # first call: the I picture to all four streams
        before = L.dsvg_ctx_decoder_redone(d.ctx)
        _, status, fnum = d.decode([pk[ii]] * S, out=dev, on_device=True)
        assert status == [0] * S
        first = d.download(dev)
        for s in range(S):
            assert np.array_equal(first[s], expected(0)), "I picture, stream %d" % s
        assert L.dsvg_ctx_decoder_redone(d.ctx) - before == 0
        # between the calls: everything settled, a sentinel over the whole buffer
        d.sync()
        sentinel = np.random.default_rng(0x5E71).integers(0, 256, (S, d.frame_bytes), dtype=np.uint8)
        assert L.dsvg_dev_upload(d.ctx, dev, sentinel.ctypes.data, sentinel.nbytes) == 0
        d.sync()
        # second call: the P picture with its symbol beyond int16 to streams 0 and 2, end of stream to 1 and 3
        before = L.dsvg_ctx_decoder_redone(d.ctx)
        _, status, fnum = d.decode([pk[ip], eos, pk[ip], eos], out=dev, on_device=True)
        assert status[0] == 0 and status[2] == 0 and status[1] in (2, 3) and status[3] in (2, 3)
        frames = d.download(dev)
        exp = expected(1)
        for s in (0, 2):
            assert np.array_equal(frames[s], exp), "stream %d: first difference at %s" % (s, np.argwhere(frames[s] != exp)[:3].ravel())
        for s in (1, 3):
            assert np.array_equal(frames[s], sentinel[s]), "stream %d: its frame was written at %s" % (s, np.argwhere(frames[s] != sentinel[s])[:3].ravel())
        assert L.dsvg_ctx_decoder_redone(d.ctx) - before == 1
    finally:
        d.close()


def test_refusals(pkg, orc):
    w, h, fmt = 352, 288, A.SUBSAMP_420
    L = pkg.lib()
    _, packets, want = streams_of(w, h, fmt)
    nv12 = PF.pf(PF.SEMI_UV)
    fb = PF.frame_bytes(nv12, w, h, fmt)
    d = pkg.DecBatch(w, h, fmt, 1)
    try:
        d.set_output_format(cpf(pkg, PF.pf(PF.SEMI_UV, 10, 1)))
        assert d.frame_bytes == 2 * fb
        d.set_output_format(cpf(pkg, nv12))
        for bad, osub in [(PF.pf(PF.YUYV), fmt), (nv12, A.SUBSAMP_444), (nv12, A.SUBSAMP_422), (PF.pf(), A.SUBSAMP_411), (PF.pf(PF.SEMI_UV, 9), fmt),
                          (PF.pf(PF.SEMI_UV, pitch=(w - 1, 0, 0)), fmt), (PF.pf(PF.SEMI_UV, frame_bytes=fb - 1), fmt)]:
            assert L.dsv1_decbatch_set_output_format(d.h, C.byref(cpf(pkg, bad)), osub) == DSVG_ERR_ARG, (bad, osub)
            with pytest.raises(ValueError):
                d.set_output_format(cpf(pkg, bad), osub)
            assert d.frame_bytes == fb == L.dsv1_decbatch_out_frame_bytes(d.h)
        # the setting in force is still NV12: decode says so
        out = np.full((1, fb), 0x5A, dtype=np.uint8)
        t = 0
        status, fnum = (C.c_int * 1)(), (C.c_uint32 * 1)()
        for p in packets[0][:3]:
            buf = (pkg.Buf * 1)()
            keep = np.frombuffer(bytes(p) + b"\0" * 16, dtype=np.uint8).copy()
            buf[0].data, buf[0].len = keep.ctypes.data_as(C.POINTER(C.c_uint8)), len(p)
            if p[5] & 4:                                 # an output pitch below the frame: refused, nothing written
                held = out.copy()                        # (the sentinel, or the picture of the call before)
                assert L.dsv1_decbatch_decode(d.h, buf, out.ctypes.data, fb - 1, 0, status, fnum) == DSVG_ERR_ARG
                assert np.array_equal(out, held)
            assert L.dsv1_decbatch_decode(d.h, buf, out.ctypes.data, 0, 0, status, fnum) == 0
            if p[5] & 4:
                assert status[0] == 0
                assert np.array_equal(out[0], PO.export(want[0][t][None], nv12, w, h, fmt, fmt, 1))
                t += 1
        assert t >= 1
    finally:
        d.close()
    assert not d.h                                       # closed: the handle is gone, and a NULL handle is refused
    assert L.dsv1_decbatch_set_output_format(d.h, C.byref(cpf(pkg, nv12)), fmt) == DSVG_ERR_ARG
    assert L.dsv1_decbatch_set_output_format(None, None, fmt) == DSVG_ERR_ARG
    with pytest.raises(ValueError):
        d.set_output_format(cpf(pkg, nv12))
