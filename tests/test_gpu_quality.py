"""Quality measurement of the encoder (include/dsv1_api.h dsv1_batch_sse_enable / dsv1_batch_get_sse, include/dsvg.h dsvg_ctx_sse_enable,
csrc/k_quality.hip): per picture and plane the exact sum of squared errors between the source and the reconstruction, computed on the
device inside the frame steps.  The expected figures come from the oracle's reconstructions (orc_encode(.., want_recon=True), pinned to
the reference by tests/test_oracle_vs_ref.py): sum (clip - recon)^2 per plane in int64, equal for every picture.  With the measurement
on, the packets stay the oracle's."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A

pytestmark = pytest.mark.gpu

DSVG_ERR_ARG = -2


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return m


def _plane_sizes(w, h, fmt):
    cw, ch = A.chroma_dims(w, h, fmt)
    return [w * h, cw * ch, cw * ch]


def expected_sse(clip, recs, w, h, fmt):
    """[frames, 3] sum of squared errors of the oracle's reconstructions, in int64"""
    sizes = _plane_sizes(w, h, fmt)
    out = np.zeros((len(recs), 3), dtype=np.uint64)
    for t, r in enumerate(recs):
        o = 0
        for p, n in enumerate(sizes):
            d = clip[t, o:o + n].astype(np.int64) - r[o:o + n].astype(np.int64)
            out[t, p] = int((d * d).sum())
            o += n
    return out


def oracle(clips, w, h, fmt, cli):
    """per stream: (stream bytes without EOS, expected SSE [frames, 3])"""
    res = []
    for clip in clips:
        data, recs = A.orc_encode(clip, A.orc_cfg(w, h, fmt, **cli), want_recon=True, eos=False)
        assert len(recs) == clip.shape[0]
        res.append((data, expected_sse(clip, recs, w, h, fmt)))
    return res


def run(pkg, clips, w, h, fmt, cli, F, mode="host", pipelined=True, streams=0, measure=True, chains=0):
    """code the clips (one per stream) in calls of F frames; returns (stream bytes, SSE [streams, frames, 3] or None)"""
    S, n = len(clips), clips[0].shape[0]
    assert n % F == 0
    b = pkg.Batch(pkg.make_encoder_cfg(w, h, fmt, **cli), S, F, chains=chains)
    try:
        if streams:
            b.code_streams(streams)
        if measure:
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
        got, sse = [b""] * S, []

        def submit(k):
            if mode == "staged":
                b.stage(calls[k])
            b.submit(calls[k], on_device=mode in ("held", "device"), held=mode == "held")

        def take(part):
            got[:] = [g + bytes(p) for g, p in zip(got, part)]
            if measure:
                sse.append(b.sse())

        if pipelined:
            submit(0)
            for k in range(1, len(calls)):
                submit(k)                           # two batches in flight, then the older one is collected
                take(b.collect())
            take(b.collect())
        else:
            for k in range(len(calls)):
                take(b.encode(calls[k], on_device=mode in ("held", "device")))
        dropped = b.dropped_recons()[0]
    finally:
        b.close()
    return got, (np.concatenate(sse, axis=1) if measure else None), dropped


def check(got, sse, want):
    for s, (data, exp) in enumerate(want):
        assert got[s] == data, "stream %d: packets differ from the oracle's with the measurement on" % s
        bad = np.nonzero((sse[s] != exp).any(axis=1))[0]
        assert bad.size == 0, "stream %d: SSE differs at frames %s: got %s want %s" % (s, bad[:4], sse[s][bad[:2]], exp[bad[:2]])


FORMATS = [A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("w,h", [(352, 288), (250, 130)])
def test_formats_and_sizes(pkg, orc, w, h, fmt):
    """GOP 12 in calls of 6 frames, 18 frames: a GOP boundary inside the clip; the call that ends with frame 11 drops its last
    reconstruction (frame 12 starts a GOP); stream 1 has scene cuts (forced I pictures)"""
    cli = dict(qp=80, gop=12, rc_mode_cli=1, scd=1)
    clips = [A.gen_clip(w, h, fmt, 0x55E0 + s, 18, style=(0, 3)[s]) for s in range(2)]
    want = oracle(clips, w, h, fmt, cli)
    got, sse, dropped = run(pkg, clips, w, h, fmt, cli, 6)
    check(got, sse, want)
    assert dropped > 0
    assert (sse > 0).all()


@pytest.mark.parametrize("fmt", [A.SUBSAMP_420, A.SUBSAMP_444])
def test_intra_only(pkg, orc, fmt):
    """gop 0: no picture keeps a reconstruction, the inverse transform runs for the measurement only"""
    w, h = 352, 288
    cli = dict(qp=75, gop=0, rc_mode_cli=1)
    clips = [A.gen_clip(w, h, fmt, 0x1770 + s, 8, style=s) for s in range(3)]
    want = oracle(clips, w, h, fmt, cli)
    got, sse, _ = run(pkg, clips, w, h, fmt, cli, 4)
    check(got, sse, want)


def test_measurement_does_not_change_the_packets(pkg, orc):
    """the same clips with the measurement off and on: the same bytes"""
    w, h, fmt = 352, 288, A.SUBSAMP_420
    cli = dict(qp=85, gop=6, rc_mode_cli=1)
    clips = [A.gen_clip(w, h, fmt, 0x0FF0 + s, 12, style=(0, 3, 5)[s]) for s in range(3)]
    off, none, _ = run(pkg, clips, w, h, fmt, cli, 6, measure=False)
    assert none is None
    on, sse, _ = run(pkg, clips, w, h, fmt, cli, 6)
    assert on == off
    check(on, sse, oracle(clips, w, h, fmt, cli))


@pytest.mark.parametrize("mode", ["host", "staged", "device", "held"])
@pytest.mark.parametrize("pipelined", [False, True])
def test_input_forms(pkg, orc, mode, pipelined):
    """host, staged pinned host, device copied, DSV1_CLIP_HELD device (chroma and luma read in place): different clips per call"""
    w, h, fmt = 352, 288, A.SUBSAMP_420
    cli = dict(qp=85, gop=12, rc_mode_cli=1)
    clips = [A.gen_clip(w, h, fmt, 0xC11F + s, 24, style=(0, 1, 2, 3)[s]) for s in range(4)]
    got, sse, _ = run(pkg, clips, w, h, fmt, cli, 8, mode=mode, pipelined=pipelined)
    check(got, sse, oracle(clips, w, h, fmt, cli))


@pytest.mark.parametrize("streams", [1, 2])
def test_coding_streams(pkg, orc, streams):
    """GOP-aligned streams of P steps: with two coding streams every step is split in two halves, each with its own launch (and
    12 frame steps per call: the halves are enqueued by threads of their own)"""
    w, h, fmt = 352, 288, A.SUBSAMP_420
    cli = dict(qp=85, gop=12, rc_mode_cli=1, scd=0)
    clips = [A.gen_clip(w, h, fmt, 0x2570 + s, 24, style=0) for s in range(4)]
    got, sse, _ = run(pkg, clips, w, h, fmt, cli, 12, mode="held", streams=streams)
    check(got, sse, oracle(clips, w, h, fmt, cli))


@pytest.mark.parametrize("serial", [False, True])
def test_abr(pkg, orc, monkeypatch, serial):
    """device-resident rate control (dsvg_code_batch_rc) and the frame-by-frame host path (DSV1_ABR_SERIAL)"""
    if serial:
        monkeypatch.setenv("DSV1_ABR_SERIAL", "1")
    w, h, fmt = 352, 288, A.SUBSAMP_420
    cli = dict(qp=80, gop=12, rc_mode_cli=0, kbps=500, scd=1)
    clips = [A.gen_clip(w, h, fmt, 0xAB50 + s, 16, style=(0, 3, 4)[s]) for s in range(3)]
    got, sse, _ = run(pkg, clips, w, h, fmt, cli, 8)
    check(got, sse, oracle(clips, w, h, fmt, cli))


@pytest.mark.parametrize("F,chains,style", [(5, 2, 3), (8, 3, 0), (6, 1, 5)])
def test_chain_mode(pkg, orc, F, chains, style):
    """one stream, GOP-parallel chains; calls end mid-GOP (the last picture's reconstruction is carried into the next call)"""
    w, h, fmt = 352, 288, A.SUBSAMP_420
    cli = dict(qp=85, gop=12, rc_mode_cli=1, scd=1)
    clips = [A.gen_clip(w, h, fmt, 0xC4A1 + F, 4 * F, style=style)]
    got, sse, _ = run(pkg, clips, w, h, fmt, cli, F, chains=chains)
    check(got, sse, oracle(clips, w, h, fmt, cli))


def test_enabled_after_a_dropped_reconstruction_is_remedied(pkg, orc):
    """batch 1 unmeasured: its last picture (frame 5, frame number 6 would start a GOP) is coded without a reconstruction; then the
    measurement goes on and stream 0 is renumbered to 3, so frame 6 is a P picture: the dropped picture is coded again before batch 2
    (remedy_dropped) -- batch 2's figures are its own pictures', counted once"""
    w, h, fmt, gop, S = 352, 288, A.SUBSAMP_420, 6, 2
    cli = dict(qp=85, gop=gop, rc_mode_cli=1, scd=0)
    clips = [A.gen_clip(w, h, fmt, 0x3E50 + s, 2 * gop, style=s) for s in range(S)]
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
        want.append((C.string_at(out.value, n_.value), expected_sse(clips[s][gop:], recs[gop:], w, h, fmt)))
        C.CDLL(None).free(out)
        Lo.orc_enc_close(e)
    b = pkg.Batch(pkg.make_encoder_cfg(w, h, fmt, **cli), S, gop)
    try:
        calls = [np.stack([clips[s][k * gop:(k + 1) * gop] for s in range(S)]) for k in range(2)]
        first = b.encode(calls[0])
        with pytest.raises(RuntimeError):
            b.sse()                                 # batch 1 was not measured
        b.sse_enable()
        b.set_fnum(0, 3)
        second = b.encode(calls[1])
        sse = b.sse()
        dropped, remedied = b.dropped_recons()
    finally:
        b.close()
    assert remedied == 1, (dropped, remedied)
    for s in range(S):
        assert first[s] + second[s] == want[s][0], "stream %d differs" % s
        assert (sse[s] == want[s][1]).all(), (s, sse[s], want[s][1])


@pytest.mark.parametrize("w,h,fmt,S,F,ncalls,cli", [
    (1920, 1080, A.SUBSAMP_420, 2, 4, 2, dict(qp=85, gop=12, rc_mode_cli=1)),
    (3840, 2160, A.SUBSAMP_444, 1, 3, 1, dict(qp=80, gop=12, rc_mode_cli=0, kbps=40000)),
])
def test_large_pictures(pkg, orc, w, h, fmt, S, F, ncalls, cli):
    clips = [A.gen_clip(w, h, fmt, 0x1A56 + s, F * ncalls, style=s) for s in range(S)]
    got, sse, _ = run(pkg, clips, w, h, fmt, cli, F, mode="held")
    check(got, sse, oracle(clips, w, h, fmt, cli))


def test_error_contract(pkg):
    w, h, fmt, F = 176, 144, A.SUBSAMP_420, 4
    b = pkg.Batch(pkg.make_encoder_cfg(w, h, fmt, qp=85, gop=12, rc_mode_cli=1), 1, F)
    L = b.L
    buf = (C.c_uint64 * (3 * F))()
    clip = A.gen_clip(w, h, fmt, 0xE770, F).reshape(1, F, -1)
    try:
        assert L.dsv1_batch_get_sse(b.h, buf, 3 * F) == DSVG_ERR_ARG       # nothing collected yet
        b.encode(clip)
        assert L.dsv1_batch_get_sse(b.h, buf, 3 * F) == DSVG_ERR_ARG       # collected, not measured
        b.submit(clip)
        assert L.dsv1_batch_sse_enable(b.h, 1) == DSVG_ERR_ARG             # a batch in flight
        b.collect()
        assert L.dsv1_batch_sse_enable(b.h, 1) == 0
        b.encode(clip)
        assert L.dsv1_batch_get_sse(b.h, buf, 3 * F - 1) == DSVG_ERR_ARG   # no room
        assert L.dsv1_batch_get_sse(b.h, None, 3 * F) == DSVG_ERR_ARG
        assert L.dsv1_batch_get_sse(b.h, buf, 3 * F) == 0
        assert all(v > 0 for v in buf)
        b.sse_enable(False)
        b.encode(clip)
        with pytest.raises(RuntimeError):
            b.sse()                                                        # measured off again
        # the operator level: a slot coded with the measurement off is refused -- out slot F, the first picture of the last call
        # (batches alternate between two halves of the out slots: calls 2 and 4 used [F, 2F))
        ctx = C.c_void_p(b.ctx)
        slot = (C.c_int * 1)(F)
        assert L.dsvg_fetch_sse(ctx, 1, slot, buf) == DSVG_ERR_ARG
    finally:
        b.close()


def test_operator_level_fetch_per_kind(pkg):
    """dsvg_fetch_sse / dsvg_fetch_ssim on a call's first out slot: the kind that was on gives Batch's figures, the other is
    refused; a context that never measured at the source resolution refuses dsvg_fetch_xres_sse.  The out slots are the batch's
    layout (csrc/host/dsv1_enc.c, batch_submit_impl: pc->out_slot = par * N * F + t * N + s * R, par alternating from 0 with every
    submit): one stream, so the first picture of call 1 is in slot 0 and of call 2 in slot F.  Each fetch is compared with the
    Batch's own figure of that picture, so another layout fails here rather than passes."""
    w, h, fmt, F = 176, 144, A.SUBSAMP_420, 4
    b = pkg.Batch(pkg.make_encoder_cfg(w, h, fmt, qp=85, gop=12, rc_mode_cli=1), 1, F)
    L, ctx = b.L, C.c_void_p(b.ctx)
    u, i = (C.c_uint64 * 3)(), (C.c_int64 * 3)()
    clip = A.gen_clip(w, h, fmt, 0xE772, 2 * F).reshape(1, 2 * F, -1)
    try:
        b.sse_enable()
        b.encode(np.ascontiguousarray(clip[:, :F]))
        slot = (C.c_int * 1)(0)                         # batches alternate between two halves of the out slots: call 1 used [0, F)
        assert L.dsvg_fetch_sse(ctx, 1, slot, u) == 0
        assert list(u) == list(b.sse()[0, 0]) and all(v > 0 for v in u)
        assert L.dsvg_fetch_ssim(ctx, 1, slot, i) == DSVG_ERR_ARG
        b.sse_enable(False)
        b.ssim_enable()
        b.encode(np.ascontiguousarray(clip[:, F:]))
        slot = (C.c_int * 1)(F)                         # call 2: [F, 2F)
        assert L.dsvg_fetch_ssim(ctx, 1, slot, i) == 0
        assert list(i) == list(b.ssim_fx()[0, 0]) and any(v != 0 for v in i)
        assert L.dsvg_fetch_sse(ctx, 1, slot, u) == DSVG_ERR_ARG
        assert L.dsvg_fetch_xres_sse(ctx, 1, slot, u) == DSVG_ERR_ARG
    finally:
        b.close()


def test_psnr_of_a_batch(pkg):
    """Batch.psnr(): the per-plane and whole-picture dB of Batch.sse() by the module's psnr_db"""
    w, h, fmt, F = 176, 144, A.SUBSAMP_422, 4
    b = pkg.Batch(pkg.make_encoder_cfg(w, h, fmt, qp=60, gop=12, rc_mode_cli=1), 2, F)
    try:
        b.sse_enable()
        b.encode(np.stack([A.gen_clip(w, h, fmt, 0x9590 + s, F) for s in range(2)]))
        sse, db = b.sse(), b.psnr()
    finally:
        b.close()
    assert sse.dtype == np.uint64 and sse.shape == (2, F, 3)
    assert db.dtype == np.float64 and db.shape == (2, F, 4)
    n = np.array(_plane_sizes(w, h, fmt), dtype=np.float64)
    assert np.allclose(db[..., :3], 10 * np.log10(255.0 ** 2 * n / sse.astype(np.float64)))
    assert np.allclose(db[..., 3], 10 * np.log10(255.0 ** 2 * n.sum() / sse.sum(axis=-1).astype(np.float64)))
    assert (db > 20).all() and (db < 70).all()
