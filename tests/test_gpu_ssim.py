"""SSIM of the encoder's quality report (include/dsv1_api.h dsv1_batch_ssim_enable / dsv1_batch_get_ssim, include/dsvg.h
dsvg_ctx_ssim_enable, csrc/k_quality.hip k_ssim): per picture and plane the exact fixed-point sum of the 8x8 windows' SSIM at stride 4,
computed on the device inside the frame steps.  The expected figures are the numpy statement of the definition (tests/_ssim.py) over the
oracle's reconstructions (orc_encode(.., want_recon=True)), equal to the integer for every picture; with SSE on as well, one pass makes
both and the SSE must still be the exact sums.  The packets stay the oracle's."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import _ssim as Q

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return m


def expected(clip, recs, w, h, fmt):
    """([frames, 3] SSIM_FX, [frames, 3] SSE) of the oracle's reconstructions"""
    cw, ch = A.chroma_dims(w, h, fmt)
    sizes = [w * h, cw * ch, cw * ch]
    fx = np.zeros((len(recs), 3), dtype=np.int64)
    sse = np.zeros((len(recs), 3), dtype=np.uint64)
    for t, r in enumerate(recs):
        fx[t] = Q.picture_fx(clip[t], r, w, h, fmt)
        o = 0
        for p, n in enumerate(sizes):
            d = clip[t, o:o + n].astype(np.int64) - r[o:o + n].astype(np.int64)
            sse[t, p] = int((d * d).sum())
            o += n
    return fx, sse


def oracle(clips, w, h, fmt, cli):
    """per stream: (stream bytes without EOS, SSIM_FX [frames, 3], SSE [frames, 3])"""
    res = []
    for clip in clips:
        data, recs = A.orc_encode(clip, A.orc_cfg(w, h, fmt, **cli), want_recon=True, eos=False)
        assert len(recs) == clip.shape[0]
        res.append((data,) + expected(clip, recs, w, h, fmt))
    return res


def run(pkg, clips, w, h, fmt, cli, F, mode="host", pipelined=True, streams=0, ssim=True, sse=False, chains=0):
    """code the clips (one per stream) in calls of F frames; returns (stream bytes, SSIM_FX [streams, frames, 3] or None,
    SSE [streams, frames, 3] or None)"""
    S, n = len(clips), clips[0].shape[0]
    assert n % F == 0
    b = pkg.Batch(pkg.make_encoder_cfg(w, h, fmt, **cli), S, F, chains=chains)
    try:
        if streams:
            b.code_streams(streams)
        if ssim:
            b.ssim_enable()
        if sse:
            b.sse_enable()
        calls = [np.ascontiguousarray(np.stack([c[k * F:(k + 1) * F] for c in clips])) for k in range(n // F)]
        if mode in ("held", "device"):
            calls = [b.upload(c) for c in calls]
        elif mode == "staged":
            pins = []
            for c in calls:
                p = b.pinned(c.shape)
                p[...] = c
                pins.append(p)
            calls = pins
        got, fx, es = [b""] * S, [], []

        def submit(k):
            if mode == "staged":
                b.stage(calls[k])
            b.submit(calls[k], on_device=mode in ("held", "device"), held=mode == "held")

        def take(part):
            got[:] = [g + bytes(p) for g, p in zip(got, part)]
            if ssim:
                fx.append(b.ssim_fx())
            if sse:
                es.append(b.sse())

        if pipelined:
            submit(0)
            for k in range(1, len(calls)):
                submit(k)                           # two batches in flight, then the older one is collected
                take(b.collect())
            take(b.collect())
        else:
            for k in range(len(calls)):
                take(b.encode(calls[k], on_device=mode in ("held", "device")))
    finally:
        b.close()
    return got, (np.concatenate(fx, axis=1) if ssim else None), (np.concatenate(es, axis=1) if sse else None)


def check(got, fx, want, sse=None):
    for s, (data, exp, exp_sse) in enumerate(want):
        assert got[s] == data, "stream %d: packets differ from the oracle's with the measurement on" % s
        bad = np.nonzero((fx[s] != exp).any(axis=1))[0]
        assert bad.size == 0, "stream %d: SSIM_FX differs at frames %s: got %s want %s" % (s, bad[:4], fx[s][bad[:2]], exp[bad[:2]])
        if sse is not None:
            bad = np.nonzero((sse[s] != exp_sse).any(axis=1))[0]
            assert bad.size == 0, "stream %d: SSE differs at frames %s: got %s want %s" % (s, bad[:4], sse[s][bad[:2]], exp_sse[bad[:2]])


FORMATS = [A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("w,h", [(352, 288), (250, 130)])
@pytest.mark.parametrize("with_sse", [False, True])
def test_formats_and_sizes(pkg, orc, w, h, fmt, with_sse):
    """GOP 12 in calls of 6 frames, 18 frames: a GOP boundary inside the clip, a dropped reconstruction; stream 1 has scene cuts.
    with_sse: both measurements on, made by one pass"""
    cli = dict(qp=80, gop=12, rc_mode_cli=1, scd=1)
    clips = [A.gen_clip(w, h, fmt, 0x5510 + s, 18, style=(0, 3)[s]) for s in range(2)]
    want = oracle(clips, w, h, fmt, cli)
    got, fx, sse = run(pkg, clips, w, h, fmt, cli, 6, sse=with_sse)
    check(got, fx, want, sse)
    one = np.array([Q.ONE * n for n in pkg.ssim_windows(w, h, fmt)], dtype=np.int64)
    assert (fx < one).all() and (fx > 0).all()


@pytest.mark.parametrize("w,h", [(32, 32), (40, 32)])
@pytest.mark.parametrize("with_sse", [False, True])
def test_smallest_pictures(pkg, orc, w, h, with_sse):
    """4:1:1 at the smallest sizes: 8- and 10-wide chroma planes, one column of windows"""
    fmt = A.SUBSAMP_411
    cli = dict(qp=70, gop=4, rc_mode_cli=1)
    clips = [A.gen_clip(w, h, fmt, 0x3232 + s, 8, style=s) for s in range(3)]
    got, fx, sse = run(pkg, clips, w, h, fmt, cli, 4, sse=with_sse)
    check(got, fx, oracle(clips, w, h, fmt, cli), sse)


@pytest.mark.parametrize("fmt", [A.SUBSAMP_420, A.SUBSAMP_444])
def test_intra_only(pkg, orc, fmt):
    """gop 0: no picture keeps a reconstruction, the inverse transform runs for the measurement only"""
    w, h = 352, 288
    cli = dict(qp=75, gop=0, rc_mode_cli=1)
    clips = [A.gen_clip(w, h, fmt, 0x1771 + s, 8, style=s) for s in range(3)]
    got, fx, _ = run(pkg, clips, w, h, fmt, cli, 4)
    check(got, fx, oracle(clips, w, h, fmt, cli))


def test_sse_is_the_same_with_ssim_on(pkg, orc):
    """SSE only (k_sse) and SSE + SSIM (one k_ssim pass): the same SSE to the bit, the same packets; SSIM alone: the same SSIM"""
    w, h, fmt = 250, 130, A.SUBSAMP_420
    cli = dict(qp=85, gop=6, rc_mode_cli=1, scd=1)
    clips = [A.gen_clip(w, h, fmt, 0x0FF1 + s, 12, style=(0, 3, 5)[s]) for s in range(3)]
    p_sse, _, sse_only = run(pkg, clips, w, h, fmt, cli, 6, ssim=False, sse=True)
    p_both, fx_both, sse_both = run(pkg, clips, w, h, fmt, cli, 6, ssim=True, sse=True)
    p_ssim, fx_only, _ = run(pkg, clips, w, h, fmt, cli, 6, ssim=True, sse=False)
    p_off, _, _ = run(pkg, clips, w, h, fmt, cli, 6, ssim=False, sse=False)
    assert p_sse == p_both == p_ssim == p_off
    assert sse_only.dtype == sse_both.dtype == np.uint64 and (sse_only == sse_both).all()
    assert (fx_both == fx_only).all()
    check(p_both, fx_both, oracle(clips, w, h, fmt, cli), sse_both)


@pytest.mark.parametrize("mode", ["host", "staged", "device", "held"])
@pytest.mark.parametrize("pipelined", [False, True])
def test_input_forms(pkg, orc, mode, pipelined):
    """host, staged pinned host, device copied, DSV1_CLIP_HELD device (chroma and luma read in place): different clips per call"""
    w, h, fmt = 352, 288, A.SUBSAMP_420
    cli = dict(qp=85, gop=12, rc_mode_cli=1)
    clips = [A.gen_clip(w, h, fmt, 0xC120 + s, 24, style=(0, 1, 2, 3)[s]) for s in range(4)]
    got, fx, _ = run(pkg, clips, w, h, fmt, cli, 8, mode=mode, pipelined=pipelined)
    check(got, fx, oracle(clips, w, h, fmt, cli))


def test_held_clip_with_odd_rows(pkg, orc):
    """a held clip whose rows are not 16-byte aligned (250 wide): the kernel's byte-wise path, SSE and SSIM"""
    w, h, fmt = 250, 130, A.SUBSAMP_422
    cli = dict(qp=85, gop=12, rc_mode_cli=1)
    clips = [A.gen_clip(w, h, fmt, 0x0DD0 + s, 12, style=s) for s in range(2)]
    got, fx, sse = run(pkg, clips, w, h, fmt, cli, 6, mode="held", sse=True)
    check(got, fx, oracle(clips, w, h, fmt, cli), sse)


@pytest.mark.parametrize("streams", [1, 2])
def test_coding_streams(pkg, orc, streams):
    """GOP-aligned streams of P steps: with two coding streams every step is split in two halves, each with its own launch"""
    w, h, fmt = 352, 288, A.SUBSAMP_420
    cli = dict(qp=85, gop=12, rc_mode_cli=1, scd=0)
    clips = [A.gen_clip(w, h, fmt, 0x2571 + s, 24, style=0) for s in range(4)]
    got, fx, sse = run(pkg, clips, w, h, fmt, cli, 12, mode="held", streams=streams, sse=streams == 2)
    check(got, fx, oracle(clips, w, h, fmt, cli), sse)


@pytest.mark.parametrize("serial", [False, True])
def test_abr(pkg, orc, monkeypatch, serial):
    """device-resident rate control (dsvg_code_batch_rc) and the frame-by-frame host path (DSV1_ABR_SERIAL)"""
    if serial:
        monkeypatch.setenv("DSV1_ABR_SERIAL", "1")
    w, h, fmt = 352, 288, A.SUBSAMP_420
    cli = dict(qp=80, gop=12, rc_mode_cli=0, kbps=500, scd=1)
    clips = [A.gen_clip(w, h, fmt, 0xAB51 + s, 16, style=(0, 3, 4)[s]) for s in range(3)]
    got, fx, sse = run(pkg, clips, w, h, fmt, cli, 8, sse=serial)
    check(got, fx, oracle(clips, w, h, fmt, cli), sse)


@pytest.mark.parametrize("F,chains,style", [(5, 2, 3), (8, 3, 0), (6, 1, 5)])
def test_chain_mode(pkg, orc, F, chains, style):
    """one stream, GOP-parallel chains; calls end mid-GOP (the last picture's reconstruction is carried into the next call)"""
    w, h, fmt = 352, 288, A.SUBSAMP_420
    cli = dict(qp=85, gop=12, rc_mode_cli=1, scd=1)
    clips = [A.gen_clip(w, h, fmt, 0xC4A2 + F, 4 * F, style=style)]
    got, fx, _ = run(pkg, clips, w, h, fmt, cli, F, chains=chains)
    check(got, fx, oracle(clips, w, h, fmt, cli))


def test_enabled_after_a_dropped_reconstruction_is_remedied(pkg, orc):
    """batch 1 unmeasured: its last picture is coded without a reconstruction; then SSIM goes on and stream 0 is renumbered so that
    frame 6 is a P picture: the dropped picture is coded again before batch 2 (remedy_dropped) -- batch 2's figures are its own
    pictures', counted once"""
    w, h, fmt, gop, S = 352, 288, A.SUBSAMP_420, 6, 2
    cli = dict(qp=85, gop=gop, rc_mode_cli=1, scd=0)
    clips = [A.gen_clip(w, h, fmt, 0x3E51 + s, 2 * gop, style=s) for s in range(S)]
    Lo = A.load_orc()
    want = []
    for s in range(S):
        cfg = A.orc_cfg(w, h, fmt, **cli)
        e = Lo.orc_enc_open(C.byref(cfg))
        out, n_, cap = C.c_void_p(None), C.c_size_t(0), C.c_size_t(0)
        Lo.orc_enc_set_next_fnum(e, 0)
        recs = []
        for t in range(2 * gop):
            if t == gop and s == 0:
                Lo.orc_enc_set_next_fnum(e, 3)
            rec = np.empty(clips[s].shape[1], dtype=np.uint8)
            Lo.orc_enc_frame(e, clips[s][t].ctypes.data, C.byref(out), C.byref(n_), C.byref(cap), rec.ctypes.data)
            recs.append(rec)
        want.append((C.string_at(out.value, n_.value),) + expected(clips[s][gop:], recs[gop:], w, h, fmt))
        C.CDLL(None).free(out)
        Lo.orc_enc_close(e)
    b = pkg.Batch(pkg.make_encoder_cfg(w, h, fmt, **cli), S, gop)
    try:
        calls = [np.stack([clips[s][k * gop:(k + 1) * gop] for s in range(S)]) for k in range(2)]
        first = b.encode(calls[0])
        with pytest.raises(RuntimeError):
            b.ssim_fx()                             # batch 1 was not measured
        b.ssim_enable()
        b.sse_enable()
        b.set_fnum(0, 3)
        second = b.encode(calls[1])
        fx, sse = b.ssim_fx(), b.sse()
        dropped, remedied = b.dropped_recons()
    finally:
        b.close()
    assert remedied == 1, (dropped, remedied)
    for s in range(S):
        assert first[s] + second[s] == want[s][0], "stream %d differs" % s
        assert (fx[s] == want[s][1]).all(), (s, fx[s], want[s][1])
        assert (sse[s] == want[s][2]).all(), (s, sse[s], want[s][2])


@pytest.mark.parametrize("w,h,fmt,S,F,ncalls,cli,with_sse", [
    (1920, 1080, A.SUBSAMP_420, 2, 4, 2, dict(qp=85, gop=12, rc_mode_cli=1), True),
    (3840, 2160, A.SUBSAMP_444, 1, 3, 1, dict(qp=80, gop=12, rc_mode_cli=0, kbps=40000), False),
])
def test_large_pictures(pkg, orc, w, h, fmt, S, F, ncalls, cli, with_sse):
    clips = [A.gen_clip(w, h, fmt, 0x1A57 + s, F * ncalls, style=s) for s in range(S)]
    got, fx, sse = run(pkg, clips, w, h, fmt, cli, F, mode="held", sse=with_sse)
    check(got, fx, oracle(clips, w, h, fmt, cli), sse)


def test_error_contract(pkg):
    w, h, fmt, F = 176, 144, A.SUBSAMP_420, 4
    b = pkg.Batch(pkg.make_encoder_cfg(w, h, fmt, qp=85, gop=12, rc_mode_cli=1), 1, F)
    L = b.L
    L.dsvg_fetch_ssim.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    buf = (C.c_int64 * (3 * F))()
    clip = A.gen_clip(w, h, fmt, 0xE771, F).reshape(1, F, -1)
    try:
        assert L.dsv1_batch_get_ssim(b.h, buf, 3 * F) == DSVG_ERR_ARG      # nothing collected yet
        b.encode(clip)
        assert L.dsv1_batch_get_ssim(b.h, buf, 3 * F) == DSVG_ERR_ARG      # collected, not measured
        b.sse_enable()
        b.encode(clip)
        assert L.dsv1_batch_get_ssim(b.h, buf, 3 * F) == DSVG_ERR_ARG      # SSE on is not SSIM on
        b.submit(clip)
        assert L.dsv1_batch_ssim_enable(b.h, 1) == DSVG_ERR_ARG            # a batch in flight
        b.collect()
        b.sse_enable(False)
        assert L.dsv1_batch_ssim_enable(b.h, 1) == 0
        b.encode(clip)
        assert L.dsv1_batch_get_ssim(b.h, buf, 3 * F - 1) == DSVG_ERR_ARG  # no room
        assert L.dsv1_batch_get_ssim(b.h, None, 3 * F) == DSVG_ERR_ARG
        assert L.dsv1_batch_get_ssim(b.h, buf, 3 * F) == 0
        one = [Q.ONE * n for n in pkg.ssim_windows(w, h, fmt)]
        assert all(0 < buf[3 * t + p] < one[p] for t in range(F) for p in range(3))
        with pytest.raises(RuntimeError):
            b.sse()                                                        # SSIM on is not SSE on
        ctx = C.c_void_p(b.ctx)
        # the operator level: out slot F holds the first picture of the last call (batches alternate between two halves of the
        # out slots), measured; an out-of-range slot is refused
        slot = (C.c_int * 1)(F)
        assert L.dsvg_fetch_ssim(ctx, 1, slot, buf) == 0 and buf[0] == b.ssim_fx()[0, 0, 0]
        assert L.dsvg_fetch_ssim(ctx, 1, (C.c_int * 1)(-1), buf) == DSVG_ERR_ARG
        assert L.dsvg_fetch_ssim(ctx, 1, (C.c_int * 1)(1 << 20), buf) == DSVG_ERR_ARG
        b.ssim_enable(False)
        b.encode(clip)
        with pytest.raises(RuntimeError):
            b.ssim()                                                       # measured off again
        assert L.dsvg_fetch_ssim(ctx, 1, (C.c_int * 1)(0), buf) == DSVG_ERR_ARG   # out slot 0: the last call's, SSIM off
    finally:
        b.close()


def test_ssim_of_a_batch(pkg):
    """Batch.ssim(): the per-plane and window-weighted whole-picture mean of Batch.ssim_fx() by the module's ssim_mean"""
    w, h, fmt, F = 176, 144, A.SUBSAMP_422, 4
    b = pkg.Batch(pkg.make_encoder_cfg(w, h, fmt, qp=60, gop=12, rc_mode_cli=1), 2, F)
    try:
        b.ssim_enable()
        b.encode(np.stack([A.gen_clip(w, h, fmt, 0x9591 + s, F) for s in range(2)]))
        fx, m = b.ssim_fx(), b.ssim()
    finally:
        b.close()
    assert fx.dtype == np.int64 and fx.shape == (2, F, 3)
    assert m.dtype == np.float64 and m.shape == (2, F, 4)
    n = np.array(pkg.ssim_windows(w, h, fmt), dtype=np.float64)
    assert np.allclose(m[..., :3], fx / (2.0 ** 32 * n))
    assert np.allclose(m[..., 3], fx.sum(axis=-1) / (2.0 ** 32 * n.sum()))
    assert (m > 0.3).all() and (m < 1).all()
    assert np.isfinite(pkg.ssim_db(m)).all()
