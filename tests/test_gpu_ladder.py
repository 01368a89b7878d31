"""Quality ladders (include/dsv1_api.h dsv1_ladder_open, Python Ladder / encode_ladder): nsources sources, each coded at nrungs rate
settings from one upload and one analysis.  Output stream k = s * nrungs + r must be byte for byte the oracle's stream of source s
with rung r's settings, and its per-picture SSE / SSIM the figures of the oracle's reconstructions (tests/test_gpu_quality.py,
tests/test_gpu_ssim.py).  The analysis runs once per source: the source-only kernels move the same bytes at 1 and 3 rungs."""
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


def expected(clip, recs, w, h, fmt, ssim):
    """([frames, 3] SSE, [frames, 3] SSIM_FX or None) of the oracle's reconstructions"""
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


def oracle(clips, w, h, fmt, base, rungs, changes=None, ssim=True):
    """[k] = (stream bytes without EOS, SSE, SSIM_FX) for source k // R at rung k % R; changes: {k: orc_encode changes}"""
    out = []
    for s, clip in enumerate(clips):
        for r, rung in enumerate(rungs):
            k = s * len(rungs) + r
            data, recs = A.orc_encode(clip, A.orc_cfg(w, h, fmt, **dict(base, **rung)), want_recon=True, eos=False,
                                      changes=(changes or {}).get(k))
            out.append((data,) + expected(clip, recs, w, h, fmt, ssim))
    return out


def run(pkg, clips, w, h, fmt, base, rungs, F, mode="host", pipelined=True, streams=0, ssim=True, between=None):
    """code the clips (one per source) at every rung in calls of F frames -> (streams, SSE [N, frames, 3], SSIM_FX or None, ladder
    counters (dropped, remedied)); between(b, k): called before the submit of call k >= 1"""
    S, n = len(clips), clips[0].shape[0]
    assert n % F == 0
    b = pkg.Ladder([pkg.make_encoder_cfg(w, h, fmt, **dict(base, **r)) for r in rungs], S, F)
    try:
        assert b.L.dsv1_batch_rungs(b.h) == len(rungs)
        if streams:
            b.code_streams(streams)
        b.sse_enable()
        if ssim:
            b.ssim_enable()
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
        got, sse, fx = [b""] * b.nstreams, [], []

        def submit(k):
            if k and between:
                between(b, k)
            if mode == "staged":
                b.stage(calls[k])
            b.submit(calls[k], on_device=mode in ("held", "device"), held=mode == "held")

        def take(part):
            assert len(part) == b.nstreams
            got[:] = [g + bytes(p) for g, p in zip(got, part)]
            sse.append(b.sse())
            if ssim:
                fx.append(b.ssim_fx())

        if pipelined:
            submit(0)
            for k in range(1, len(calls)):
                submit(k)
                take(b.collect())
            take(b.collect())
        else:
            for k in range(len(calls)):
                if k and between:
                    between(b, k)
                take(b.encode(calls[k], on_device=mode in ("held", "device")))
        counters = b.dropped_recons()
    finally:
        b.close()
    return got, np.concatenate(sse, axis=1), (np.concatenate(fx, axis=1) if ssim else None), counters


def check(got, sse, fx, want):
    assert len(got) == len(want)
    for k, (data, esse, efx) in enumerate(want):
        assert got[k] == data, "output stream %d: packets differ from the oracle's" % k
        bad = np.nonzero((sse[k] != esse).any(axis=1))[0]
        assert bad.size == 0, "output stream %d: SSE differs at frames %s" % (k, bad[:4])
        if fx is not None:
            bad = np.nonzero((fx[k] != efx).any(axis=1))[0]
            assert bad.size == 0, "output stream %d: SSIM differs at frames %s" % (k, bad[:4])


CRF4 = [dict(qp=30), dict(qp=60), dict(qp=85), dict(qp=95)]
FORMATS = [A.SUBSAMP_444, A.SUBSAMP_422, A.SUBSAMP_420, A.SUBSAMP_411]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("w,h", [(352, 288), (250, 130)])
def test_formats_and_sizes(pkg, orc, w, h, fmt):
    """four CRF rungs, two sources (source 1 with scene cuts), GOP 12 in calls of 6 frames over 18 frames"""
    base = dict(gop=12, rc_mode_cli=1, scd=1)
    clips = [A.gen_clip(w, h, fmt, 0x1AD0 + s, 18, style=(0, 3)[s]) for s in range(2)]
    got, sse, fx, _ = run(pkg, clips, w, h, fmt, base, CRF4, 6)
    check(got, sse, fx, oracle(clips, w, h, fmt, base, CRF4))


@pytest.mark.parametrize("gop,F,n,style", [(0, 4, 8, 1), (30, 8, 24, 3), (12, 12, 24, 5)])
def test_gop_structures(pkg, orc, gop, F, n, style):
    """intra-only; a GOP longer than a call with scene cuts; whole GOPs per call"""
    w, h, fmt = 352, 288, A.SUBSAMP_420
    base = dict(gop=gop, rc_mode_cli=1, scd=1)
    rungs = CRF4[1:]
    clips = [A.gen_clip(w, h, fmt, 0x6070 + s, n, style=(style, 0)[s]) for s in range(2)]
    got, sse, fx, _ = run(pkg, clips, w, h, fmt, base, rungs, F)
    check(got, sse, fx, oracle(clips, w, h, fmt, base, rungs))


@pytest.mark.parametrize("serial", [False, True])
def test_abr_rungs_and_a_bitrate_change(pkg, orc, monkeypatch, serial):
    """ABR rungs at different rates, device-resident rate control and DSV1_ABR_SERIAL; rung 1 of every source gets a new bitrate
    before the second call"""
    if serial:
        monkeypatch.setenv("DSV1_ABR_SERIAL", "1")
    w, h, fmt, F = 352, 288, A.SUBSAMP_420, 8
    base = dict(qp=80, gop=12, rc_mode_cli=0, scd=1)
    rungs = [dict(kbps=300), dict(kbps=700), dict(kbps=1500)]
    clips = [A.gen_clip(w, h, fmt, 0xAB1D + s, 16, style=(0, 4)[s]) for s in range(2)]
    new_rate = 1100 * 1024

    def between(b, k):
        for s in range(len(clips)):
            b.encoder(b.stream(s, 1)).bitrate = new_rate

    got, sse, fx, _ = run(pkg, clips, w, h, fmt, base, rungs, F, between=between)
    changes = {s * 3 + 1: {F: {"bitrate": new_rate}} for s in range(len(clips))}
    check(got, sse, fx, oracle(clips, w, h, fmt, base, rungs, changes))


def test_force_metadata_on_one_rung_starts_a_gop_on_every_rung(pkg, orc):
    w, h, fmt, F = 352, 288, A.SUBSAMP_420, 5
    base = dict(gop=12, rc_mode_cli=1, scd=0)
    rungs = CRF4[:3]
    clips = [A.gen_clip(w, h, fmt, 0xF04C + s, 15, style=s) for s in range(2)]

    def between(b, k):
        if k == 1:
            pkg.lib().dsv_enc_force_metadata(C.c_void_p(C.addressof(b.encoder(b.stream(0, 2)))))

    got, sse, fx, _ = run(pkg, clips, w, h, fmt, base, rungs, F, between=between)
    changes = {r: {F: {"force_metadata": True}} for r in range(3)}            # every rung of source 0
    want = oracle(clips, w, h, fmt, base, rungs, changes)
    check(got, sse, fx, want)
    assert want[0][0] != oracle(clips[:1], w, h, fmt, base, rungs[:1], ssim=False)[0][0]      # (the GOP start shows)


def test_set_fnum_remedy(pkg, orc):
    """call 1 drops the last reconstruction of every output (frame number 6 starts a GOP); stream 4 (source 1, rung 1) is renumbered
    to 3, so every rung of source 1 finds a P picture there: the dropped pictures are coded again, once per rung"""
    w, h, fmt, gop, S, R = 352, 288, A.SUBSAMP_420, 6, 2, 3
    base = dict(gop=gop, rc_mode_cli=1, scd=0)
    rungs = CRF4[1:]
    clips = [A.gen_clip(w, h, fmt, 0x5EF0 + s, 2 * gop, style=s) for s in range(S)]
    Lo = A.load_orc()
    want = []
    for s in range(S):
        for rung in rungs:
            e = Lo.orc_enc_open(C.byref(A.orc_cfg(w, h, fmt, **dict(base, **rung))))
            out, n_, cap = C.c_void_p(None), C.c_size_t(0), C.c_size_t(0)
            Lo.orc_enc_set_next_fnum(e, 0)
            recs = []
            for t in range(2 * gop):
                if t == gop and s == 1:
                    Lo.orc_enc_set_next_fnum(e, 3)
                rec = np.empty(clips[s].shape[1], dtype=np.uint8)
                Lo.orc_enc_frame(e, clips[s][t].ctypes.data, C.byref(out), C.byref(n_), C.byref(cap), rec.ctypes.data)
                recs.append(rec)
            want.append((C.string_at(out.value, n_.value), expected(clips[s][gop:], recs[gop:], w, h, fmt, False)[0]))
            C.CDLL(None).free(out)
            Lo.orc_enc_close(e)
    b = pkg.Ladder([pkg.make_encoder_cfg(w, h, fmt, **dict(base, **r)) for r in rungs], S, gop)
    try:
        calls = [np.stack([clips[s][k * gop:(k + 1) * gop] for s in range(S)]) for k in range(2)]
        first = b.encode(calls[0])
        b.sse_enable()
        b.set_fnum(b.stream(1, 1), 3)
        assert [b.encoder(k).next_fnum for k in range(S * R)] == [gop] * R + [3] * R
        second = b.encode(calls[1])
        sse = b.sse()
        dropped, remedied = b.dropped_recons()
    finally:
        b.close()
    assert remedied == R, (dropped, remedied)
    for k in range(S * R):
        assert first[k] + second[k] == want[k][0], "output stream %d differs" % k
        assert (sse[k] == want[k][1]).all(), k


@pytest.mark.parametrize("mode", ["host", "staged", "device", "held"])
def test_input_forms_pipelined(pkg, orc, mode):
    w, h, fmt = 352, 288, A.SUBSAMP_420
    base = dict(gop=12, rc_mode_cli=1)
    rungs = [dict(qp=50), dict(qp=90)]
    clips = [A.gen_clip(w, h, fmt, 0x1F0F + s, 24, style=(0, 1, 2)[s]) for s in range(3)]
    got, sse, fx, _ = run(pkg, clips, w, h, fmt, base, rungs, 8, mode=mode)
    check(got, sse, fx, oracle(clips, w, h, fmt, base, rungs))


def test_encode_calls(pkg, orc):
    """the non-pipelined form (dsv1_batch_encode) and encode_ladder"""
    w, h, fmt = 176, 144, A.SUBSAMP_422
    base = dict(gop=6, rc_mode_cli=1)
    rungs = [dict(qp=40), dict(qp=70), dict(qp=95)]
    clips = [A.gen_clip(w, h, fmt, 0xE0C0 + s, 12, style=s) for s in range(2)]
    got, sse, fx, _ = run(pkg, clips, w, h, fmt, base, rungs, 6, pipelined=False)
    check(got, sse, fx, oracle(clips, w, h, fmt, base, rungs))
    one = pkg.encode_ladder(clips[0], w, h, fmt, rungs, **base)
    assert one == [A.orc_encode(clips[0], A.orc_cfg(w, h, fmt, **dict(base, **r)))[0] for r in rungs]


@pytest.mark.parametrize("streams", [1, 2])
def test_coding_streams(pkg, orc, streams):
    w, h, fmt = 352, 288, A.SUBSAMP_420
    base = dict(gop=12, rc_mode_cli=1, scd=0)
    clips = [A.gen_clip(w, h, fmt, 0x25C0 + s, 24, style=0) for s in range(2)]
    got, sse, fx, _ = run(pkg, clips, w, h, fmt, base, CRF4[1:], 12, mode="held", streams=streams)
    check(got, sse, fx, oracle(clips, w, h, fmt, base, CRF4[1:]))


def test_1080p(pkg, orc):
    w, h, fmt = 1920, 1080, A.SUBSAMP_420
    base = dict(gop=12, rc_mode_cli=1)
    rungs = [dict(qp=60), dict(qp=85), dict(qp=95)]
    clips = [A.gen_clip(w, h, fmt, 0x1080 + s, 8, style=s) for s in range(2)]
    got, sse, _, _ = run(pkg, clips, w, h, fmt, base, rungs, 4, mode="held", ssim=False)
    check(got, sse, None, oracle(clips, w, h, fmt, base, rungs, ssim=False))


@pytest.mark.parametrize("cli", [dict(qp=85, gop=12, rc_mode_cli=1), dict(qp=80, gop=12, rc_mode_cli=0, kbps=600)])
def test_one_rung_is_a_plain_batch(pkg, orc, cli):
    w, h, fmt, F = 352, 288, A.SUBSAMP_420, 6
    clips = np.stack([A.gen_clip(w, h, fmt, 0x0AE0 + s, 2 * F, style=s) for s in range(3)])
    cfg = pkg.make_encoder_cfg(w, h, fmt, **cli)
    res = []
    for b in (pkg.Batch(cfg, 3, F), pkg.Ladder([cfg], 3, F)):
        try:
            b.sse_enable()
            out, sse = [b""] * 3, []
            for k in range(2):
                part = b.encode(np.ascontiguousarray(clips[:, k * F:(k + 1) * F]))
                out = [o + p for o, p in zip(out, part)]
                sse.append(b.sse())
            res.append((out, np.concatenate(sse, axis=1), b.L.dsv1_batch_rungs(b.h)))
        finally:
            b.close()
    assert res[0][0] == res[1][0]
    assert (res[0][1] == res[1][1]).all()
    assert res[0][2] == res[1][2] == 1


def test_analysis_runs_once(pkg):
    """the same submit at 1 and 3 rungs: the source-only kernels (frame load, motion search) move the same bytes in the same
    launches, the forward transform of P pictures three times the bytes"""
    w, h, fmt, F, S = 1920, 1080, A.SUBSAMP_420, 4, 2          # (the motion search's k_hme_csum runs on pictures this large)
    clips = np.stack([A.gen_clip(w, h, fmt, 0x0E5A + s, F, style=s) for s in range(S)])
    kernels = ["k_unpack", "void k_hme_level<true>", "k_hme_csum", "void k_fwd_mc_fast<0>"]
    got = {}
    for rungs in (CRF4[2:3], CRF4[1:]):
        b = pkg.Ladder([pkg.make_encoder_cfg(w, h, fmt, gop=12, rc_mode_cli=1, **r) for r in rungs], S, F)
        try:
            b.prof_enable(kernels)
            b.encode(clips)
            b.sync()
            got[len(rungs)] = {k: b.prof_get(k) for k in kernels}
        finally:
            b.close()
    for k in kernels[:3]:
        assert got[1][k][1] > 0, k
        assert got[3][k][1:] == got[1][k][1:], (k, got[1][k], got[3][k])
    assert got[1]["void k_fwd_mc_fast<0>"][2] > 0
    assert got[3]["void k_fwd_mc_fast<0>"][2] == pytest.approx(3 * got[1]["void k_fwd_mc_fast<0>"][2], rel=1e-9)


def test_error_contract(pkg):
    w, h, fmt, F, S = 176, 144, A.SUBSAMP_420, 4, 2
    L = pkg.lib()
    good = [pkg.make_encoder_cfg(w, h, fmt, qp=q, gop=12, rc_mode_cli=1) for q in (50, 90)]
    h_ = C.c_void_p(None)
    bad = (pkg.Encoder * 2)(good[0], pkg.make_encoder_cfg(w, h, fmt, qp=90, gop=12, rc_mode_cli=1, scd=0))
    assert L.dsv1_ladder_open(C.byref(h_), bad, 2, 0, S, F) == DSVG_ERR_ARG
    mixed = (pkg.Encoder * 2)(good[0], pkg.make_encoder_cfg(w, h, fmt, qp=90, gop=12, rc_mode_cli=0, kbps=500))
    assert L.dsv1_ladder_open(C.byref(h_), mixed, 2, 0, S, F) == DSVG_ERR_ARG
    assert L.dsv1_ladder_open(C.byref(h_), (pkg.Encoder * 17)(*([good[0]] * 17)), 17, 0, S, F) == DSVG_ERR_ARG
    assert not h_.value
    b = pkg.Ladder(good, S, F)
    try:
        clip = np.stack([A.gen_clip(w, h, fmt, 0xE770 + s, F) for s in range(S)])
        with pytest.raises(ValueError):
            b.encode(np.concatenate([clip, clip]))          # one copy per rung is not the input form
        out = b.encode(clip)
        assert len(out) == S * 2
        with pytest.raises(IndexError):
            b.encoder(S * 2)
        e = pkg.Buf()
        assert L.dsv1_batch_eos(b.h, S * 2, C.byref(e)) == DSVG_ERR_ARG
        assert L.dsv1_batch_recon_slot(b.h, S * 2) == -1
        slots = [L.dsv1_batch_recon_slot(b.h, k) for k in range(S * 2)]
        assert min(slots) >= 0 and len(set(slots)) == S * 2          # a reconstruction per output stream
        b.sse_enable()
        b.encode(clip)
        buf = (C.c_uint64 * (3 * F * S * 2))()
        assert L.dsv1_batch_get_sse(b.h, buf, 3 * F * S * 2 - 1) == DSVG_ERR_ARG
        assert L.dsv1_batch_get_sse(b.h, buf, 3 * F * S * 2) == 0
        sse = np.frombuffer(buf, dtype=np.uint64).reshape(S * 2, F, 3)
        assert (sse[0::2].sum(axis=-1) > sse[1::2].sum(axis=-1)).all()      # the coarse rung of every source has the larger errors
    finally:
        b.close()
