"""A REFUSED submit leaves the session as it found it (csrc/host/dsv1_enc.c, submit_check: every refusal that needs only the arguments
and the batch comes before a source pass runs, a staged clip is popped, a frame is loaded or a frame number is given out).

The refusal used: source-resolution figures are on and the submit is made without naming the reference clip
(dsv1_batch_xres_source).  The caller then names the clip and submits the same frames, and the next ones: packets and figures must be
those of a batch that never made the mistake, and those of the oracle's streams.  96x80 4:2:0, two streams, 4 frames per call, GOP 4,
CRF, 8 frames per stream.

An ABR stream cannot reach chain mode through the public API: dsv1_stream_open refuses every rate-control mode but CRF when the
session is opened, and the drop-in session opens chains for CRF streams only -- so `abr && chains` has no case here."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import _cabi as A
import _denoise as D
import _resample as RS
import _scale as Z

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2
W, H, FMT, S, F, N = 96, 80, A.SUBSAMP_420, 2, 4, 8
CFG = dict(gop=4, rc_mode_cli=1, scd=1)
DN = 24


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    L = m.lib()
    L.dsv1_batch_xres_enable.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.dsv1_batch_xres_source.argtypes = [C.c_void_p, C.c_void_p]
    L.dsv1_batch_get_xres_sse.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.dsv1_batch_get_xres_ssim.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    return m


@functools.lru_cache(maxsize=None)
def clips():
    return tuple(A.gen_clip(W, H, FMT, 0x5EF0 + s, N, style=1) for s in range(S))


@functools.lru_cache(maxsize=None)
def oracle(denoise):
    """per stream: (bytes without EOS, source-resolution SSE [N, 3], SSIM_FX [N, 3]) against the clip as the caller gave it"""
    out = []
    for clip in clips():
        coded = D.denoise_clip(clip, W, H, FMT, DN, DN)[0] if denoise else clip
        data, recs = A.orc_encode(coded, A.orc_cfg(W, H, FMT, **CFG), want_recon=True, eos=False)
        q = [RS.src_quality(clip[t], r, W, H, W, H, FMT, Z.CUBIC) for t, r in enumerate(recs)]
        out.append((data, np.stack([a for a, _ in q]), np.stack([b for _, b in q])))
    return out


def session(pkg, mistake, denoise=False, host=False, capfd=None):
    """code the 8 frames in two calls; mistake: the first submit is made once without the reference clip named -> (streams, SSE, SSIM_FX)"""
    b = pkg.Batch(pkg.make_encoder_cfg(W, H, FMT, **CFG), S, F)
    L = b.L
    try:
        if denoise:
            b.set_source_denoise(pkg.Denoise(DN, DN))
        assert L.dsv1_batch_xres_enable(b.h, 1, 1, W, H, Z.CUBIC) == 0
        calls = [np.ascontiguousarray(np.stack([c[k * F:(k + 1) * F] for c in clips()])) for k in range(N // F)]
        devs = [b.upload(c) for c in calls]
        got, sse, fx = [b""] * S, [], []
        for k, (c, d) in enumerate(zip(calls, devs)):
            if host:
                b.stage(c)
            if mistake and k == 0:
                bufs = (pkg.Buf * S)()
                ptr, kind = (c.ctypes.data, 0) if host else (d, 1)
                assert L.dsv1_batch_submit(b.h, ptr, kind, bufs) == DSVG_ERR_ARG
                if capfd:
                    assert "source-resolution figures on, but no reference clip named for this submit" in "".join(capfd.readouterr())
                if host:
                    # the clip is still staged: another pointer is refused as ever, this one is taken below
                    assert L.dsv1_batch_xres_source(b.h, d) == 0
                    other = c.copy()
                    assert L.dsv1_batch_submit(b.h, other.ctypes.data, 0, bufs) == DSVG_ERR_ARG
                    assert "a different clip was staged for this submit" in "".join(capfd.readouterr())
            assert L.dsv1_batch_xres_source(b.h, d) == 0
            b.submit(c if host else d, on_device=not host)
            got = [g + bytes(p) for g, p in zip(got, b.collect())]
            for fn, dt, acc in ((L.dsv1_batch_get_xres_sse, np.uint64, sse), (L.dsv1_batch_get_xres_ssim, np.int64, fx)):
                v = np.zeros((S, F, 3), dtype=dt)
                assert fn(b.h, v.ctypes.data, v.size) == 0
                acc.append(v)
    finally:
        b.close()
    return got, np.concatenate(sse, axis=1), np.concatenate(fx, axis=1)


def check(pkg, denoise=False, host=False, capfd=None):
    good = session(pkg, False, denoise, host)
    got = session(pkg, True, denoise, host, capfd)
    for s, (data, esse, efx) in enumerate(oracle(denoise)):
        assert good[0][s] == data, "stream %d of the batch that made no mistake differs from the oracle's" % s
        assert got[0][s] == good[0][s], "stream %d: the refused submit changed the packets" % s
        for name, a, g, e in (("SSE", got[1], good[1], esse), ("SSIM", got[2], good[2], efx)):
            assert np.array_equal(g[s], e), "stream %d: source-resolution %s differs from the oracle's" % (s, name)
            assert np.array_equal(a[s], g[s]), "stream %d: the refused submit changed the source-resolution %s" % (s, name)


def test_reference_clip_not_named(pkg, capfd):
    check(pkg, capfd=capfd)


def test_reference_clip_not_named_behind_a_noise_filter(pkg):
    """the refused submit must not have run the source chain: the filter's state is the stream's first picture's still"""
    check(pkg, denoise=True)


def test_reference_clip_not_named_host_input_stays_staged(pkg, capfd):
    check(pkg, host=True, capfd=capfd)
