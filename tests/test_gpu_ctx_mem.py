"""A context's memory on the device (csrc/dsvg_ctx_mem.h; ctx_alloc / ctx_release / ctx_grow in csrc/dsvg_pipe.hip): what a context
holds is what dsvg_ctx_mem_plan says, lazy buffers appear with the call that needs them at the size dsvg_ctx_mem_grow says, every
allocation of a creation may fail, and destroying a context returns everything."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
import torch

import _cabi as A
import _pixfmt as PF
import _pixout as PO
import _resample as RS
from test_gpu_batch_plan import PicOut
from test_gpu_drawinfo import decoder_case, run as run_decoder
from test_gpu_pixout import cpf

pytestmark = pytest.mark.gpu

S420, S422, S444 = A.SUBSAMP_420, A.SUBSAMP_422, A.SUBSAMP_444
DSVG_ERR_HIP = -1


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    L = m._mem_lib()
    L.dsvg_ctx_create.argtypes = [C.POINTER(C.c_void_p)] + [C.c_int] * 9
    L.dsvg_ctx_destroy.argtypes = [C.c_void_p]
    L.dsvg_ctx_destroy.restype = None
    L.dsvg_ctx_sync.argtypes = [C.c_void_p]
    L.dsvg_load_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.dsvg_fetch_pictures.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(PicOut)]
    return m


def create(pkg, w, h, fmt, slots, pyramid=0):
    ctx = C.c_void_p(None)
    rc = pkg.lib().dsvg_ctx_create(C.byref(ctx), 0, w, h, fmt, pyramid, *slots)
    return rc, ctx


def lazy_names(pkg):
    names = pkg.ctx_mem_names()
    return names[names.index("ltab_d"):]


def held(live):
    """the lazy buffers a context holds: {name: bytes}"""
    return {k: v for k, v in live.items() if v}


CONTEXTS = [(g, s) for g in ((40, 32, S444), (96, 64, S420), (250, 130, S422)) for s in ((1, 1, 1, 1), (2, 3, 2, 4))] + [((96, 64, S420), (16, 16, 16, 32))]


@pytest.mark.parametrize("geom,slots", CONTEXTS, ids=["%dx%d-0x%x-%s" % (g + ("-".join(map(str, s)),)) for g, s in CONTEXTS])
def test_created_equals_planned(pkg, geom, slots):
    """((16,16,16,32): max_jobs >= 16, the context that probes its streams' hardware queues)"""
    w, h, fmt = geom
    before = pkg.mem_outstanding()
    rows, tot = pkg.ctx_mem_plan(w, h, fmt, 0, *slots)
    rc, ctx = create(pkg, w, h, fmt, slots)
    A.chk(pkg.lib(), rc)
    try:
        live = pkg.ctx_mem_live(ctx)
        assert [(r["name"], r["bytes"]) for r in rows] == [(n, live[n]) for n in pkg.ctx_mem_names() if live[n]]
        assert not any(live[n] for n in lazy_names(pkg))
        now = pkg.mem_outstanding()
        assert (now[0] - before[0], now[1] - before[1]) == (tot["device"], tot["pinned"])
    finally:
        pkg.lib().dsvg_ctx_destroy(ctx)
    assert pkg.mem_outstanding() == before


def test_host_load_and_a_fetch_of_few_pictures_on_a_bare_context(pkg):
    """dsvg_load_frames from host memory stages the frames (yuv_stage: what it asks for); dsvg_fetch_pictures of three out slots whose
    newest call is the context's newest -- here: none yet, empty payloads -- takes the one-round-trip path with its 1 MiB pair"""
    w, h, fmt = 96, 64, S420
    L = pkg.lib()
    geo = dict(w=w, h=h, fmt=fmt, n_src_slots=2, n_recon_slots=3, max_jobs=2, out_slots=4)
    rc, ctx = create(pkg, w, h, fmt, (2, 3, 2, 4))
    A.chk(L, rc)
    try:
        clip = A.gen_clip(w, h, fmt, 0xC7A, 2, style=2)
        fb = A.frame_bytes(w, h, fmt)
        A.chk(L, L.dsvg_load_frames(ctx, 0, 2, clip.ctypes.data, 0, 1))
        A.chk(L, L.dsvg_ctx_sync(ctx))
        assert held({n: pkg.ctx_mem_live(ctx)[n] for n in lazy_names(pkg)}) == {"yuv_stage": pkg.ctx_mem_grow("yuv_stage", 2 * fb, 0, **geo)} == {"yuv_stage": 2 * fb + 256}
        A.chk(L, L.dsvg_load_frames(ctx, 0, 1, clip.ctypes.data, 0, 1))         # a smaller load keeps the stage
        assert pkg.ctx_mem_live(ctx)["yuv_stage"] == 2 * fb + 256
        slots, outs = (C.c_int * 3)(0, 1, 2), (PicOut * 3)()
        A.chk(L, L.dsvg_fetch_pictures(ctx, 3, slots, outs))
        assert all(o.nbytes[p] == 0 for o in outs for p in range(3))
        mib = pkg.ctx_mem_grow("gath_d", 12 * 65536 + 64, 0, few=True, **geo)
        assert mib == 1 << 20
        assert held({n: pkg.ctx_mem_live(ctx)[n] for n in lazy_names(pkg)}) == {"yuv_stage": 2 * fb + 256, "gath_d": mib, "gath_h": mib}
    finally:
        L.dsvg_ctx_destroy(ctx)


def _serial_abr_batch(pkg, cfg, S, F):
    old = os.environ.get("DSV1_ABR_SERIAL")
    os.environ["DSV1_ABR_SERIAL"] = "1"
    try:
        return pkg.Batch(cfg, S, F)
    finally:
        if old is None:
            del os.environ["DSV1_ABR_SERIAL"]
        else:
            os.environ["DSV1_ABR_SERIAL"] = old


def test_encoder_fetches_and_measurements(pkg, orc):
    """frame-serial ABR streams fetch three pictures at a time: the I pictures of the first frame on the general path (the pair grows to
    twice the payloads + 1 MiB, more than the P pictures' one round trip asks for afterwards); the host clip goes through an ingest
    buffer and is loaded by a slot table.  Switching a measurement on allocates its table pair, and nothing else."""
    w, h, fmt, S, F, calls = 96, 64, S420, 3, 2, 2
    kw = dict(qp=60, gop=12, rc_mode_cli=0)
    geo = dict(w=w, h=h, fmt=fmt, n_src_slots=(2 * F + 1) * S, n_recon_slots=2 * S, max_jobs=S, out_slots=2 * S * F)
    clips = np.stack([A.gen_clip(w, h, fmt, 0xC7B0 + s, F * calls, style=[1, 2, 4][s]) for s in range(S)])
    want = [A.orc_encode(clips[s], A.orc_cfg(w, h, fmt, **kw), eos=False)[0] for s in range(S)]
    b = _serial_abr_batch(pkg, pkg.make_encoder_cfg(w, h, fmt, **kw), S, F)
    try:
        rows, _ = pkg.ctx_mem_plan(**{"pyramid_levels": 0, **geo})
        live = b.mem_live()
        assert [(r["name"], r["bytes"]) for r in rows] == [(n, v) for n, v in live.items() if v]
        got = [b""] * S
        for k in range(calls):
            for s, o in enumerate(b.encode(np.ascontiguousarray(clips[:, k * F:(k + 1) * F]))):
                got[s] += o
            now = held({n: b.mem_live()[n] for n in lazy_names(pkg)})
            print("serial ABR call", k, now)
            assert set(now) == {"ltab_d", "ingest0", "gath_d", "gath_h"} | ({"ingest1"} if k else set()), now
            assert now["ltab_d"] == pkg.ctx_mem_grow("ltab_d", 1, 0, **geo) == 4 * (2 * F + 1) * S + 64       # the slot table of the mapped load
            assert now["ingest0"] == S * F * A.frame_bytes(w, h, fmt) + 256 == pkg.ctx_mem_grow("ingest0", S * F * A.frame_bytes(w, h, fmt), 0, **geo)
            assert now["gath_d"] == now["gath_h"] > 1 << 20 and (now["gath_d"] - (1 << 20)) % 32 == 0
        assert got == want
    finally:
        b.close()
    kw = dict(qp=85, gop=12, rc_mode_cli=1)
    clip = A.gen_clip(w, h, fmt, 0xC7C, F, style=2)
    want, _ = A.orc_encode(clip, A.orc_cfg(w, h, fmt, **kw), eos=False)
    b = pkg.Batch(pkg.make_encoder_cfg(w, h, fmt, **kw), 1, F)
    try:
        geo = dict(w=w, h=h, fmt=fmt, n_src_slots=2 * F + 1, n_recon_slots=2, max_jobs=1, out_slots=2 * F)
        q = pkg.ctx_mem_grow("q0_dev", 1, 0, **geo), pkg.ctx_mem_grow("q0_host", 1, 0, **geo)
        assert q == (8 * 3 * 2 * F + 256, 8 * 3 * 2 * F + 64)
        b.sse_enable()
        assert held({n: b.mem_live()[n] for n in lazy_names(pkg)}) == {"q0_dev": q[0], "q0_host": q[1]}
        b.ssim_enable()
        assert held({n: b.mem_live()[n] for n in lazy_names(pkg)}) == {"q0_dev": q[0], "q0_host": q[1], "q1_dev": q[0], "q1_host": q[1]}
        assert b.encode(clip[None])[0] == want
        assert b.sse().shape == (1, F, 3) and b.ssim_fx().shape == (1, F, 3)
    finally:
        b.close()


def test_decoder_output_pass_and_overlay(pkg):
    """three streams of the draw-info fixture (tests/test_gpu_drawinfo.py: decoder_case, whose frames are the oracle's), host output.
    With a scale and NV12 on top: the payload pair of both parities, the parse records, the flags, the output table, the scaled
    scratch, the stage; the last call leaves the intra-only stream without a picture, so the pass is given output frame indices and
    pairs scratch frames with them: osc_tab_d appears there, and nothing else changes.  With the overlay: the scratch frames."""
    from _drawinfo_cases import FRAMES
    w, h, streams, pics, plain, drawn = decoder_case(pkg, "96x64", S420)
    S, (dw, dh, filt) = 3, (63, 40, RS.CUBIC)
    geo = dict(w=w, h=h, fmt=S420, pyramid_levels=1, n_src_slots=1, n_recon_slots=3 * S, max_jobs=S, out_slots=S)
    f = PF.pf(PF.SEMI_UV)
    lazy = lambda d: held({n: d.mem_live()[n] for n in lazy_names(pkg)})

    def fresh(d):
        assert not lazy(d)
        rows, _ = pkg.ctx_mem_plan(**geo)
        assert [(r["name"], r["bytes"]) for r in rows] == [(n, v) for n, v in d.mem_live().items() if v]

    fb = PF.frame_bytes(f, dw, dh, S420)
    eos = A.split_packets(streams[0])[-1]
    assert not eos[5] & 4
    tabs = 8 * 3 * S + 64                                                     # (slot or scratch frame, output frame) pairs: one per reconstruction slot
    d = pkg.DecBatch(w, h, S420, S)
    try:
        fresh(d)
        d.set_output_scale(dw, dh, filt)
        d.set_output_format(cpf(pkg, f), S420)
        assert d.frame_bytes == fb
        for k in range(FRAMES):
            partial = k == FRAMES - 1
            before = lazy(d)
            host = np.full((S, fb), 0xA5, np.uint8)                           # the sentinel
            expect = host.copy()
            _, status, fnum = d.decode([eos if partial and s == 1 else pics[s][k] for s in range(S)], out=host)
            for s in range(S):
                if partial and s == 1:
                    assert status[s] in (2, 3)                                # no picture: its frame keeps the sentinel
                    continue
                assert status[s] == 0 and fnum[s] == k
                PO.export(RS.resample_frame(plain[k, s], w, h, S420, dw, dh, filt)[None], f, dw, dh, S420, S420, 1, into=expect[s])
            A.assert_same("call %d as NV12 at %dx%d" % (k, dw, dh), host, expect)
            now = lazy(d)
            print("decoder, scale + NV12, call", k, now)
            if partial:
                assert {n: v for n, v in now.items() if before.get(n) != v} == {"osc_tab_d": tabs}
            else:
                assert "osc_tab_d" not in now
        snap = lazy(d)
    finally:
        d.close()
    fixed = {n: pkg.ctx_mem_grow(n, 1, 0, **geo) for n in ("otab_d", "osc_tab_d", "dec_flag_d", "dec_flag_h")}
    assert fixed == {"otab_d": tabs, "osc_tab_d": tabs, "dec_flag_d": 8 * S, "dec_flag_h": 8 * S}
    assert set(snap) == {"dec_h0", "dec_h1", "dec_d0", "dec_d1", "dec_meta", "dec_flag_d", "dec_flag_h", "otab_d", "osc_scratch", "osc_tab_d", "yuv_stage"}
    assert {n: snap[n] for n in fixed} == fixed
    osc_fb = (A.frame_bytes(dw, dh, S420) + 255) & ~255                      # scaled packed planar frames, 256 apart, one per reconstruction slot
    assert snap["osc_scratch"] == pkg.ctx_mem_grow("osc_scratch", osc_fb * 3 * S, 0, **geo) == osc_fb * 3 * S + 256
    assert 256 < snap["yuv_stage"] <= fb * S + 256                            # at most the call's NV12 frames at the caller's pitch
    assert snap["dec_d0"] == snap["dec_h0"] + 256 and snap["dec_h0"] > 1 << 20 and snap["dec_meta"] > 4096 * 24
    snap = {}
    got = run_decoder(pkg, w, h, S420, pics, [7] * FRAMES, setting=fresh, before_close=lambda d: snap.update(lazy(d)))
    for k in range(FRAMES):
        for s in range(S):
            A.assert_same("call %d stream %d drawn" % (k, s), got[k, s], drawn[k, s])
    print("decoder, overlay:", snap)
    assert set(snap) == {"dec_h0", "dec_h1", "dec_d0", "dec_d1", "dec_meta", "dec_flag_d", "dec_flag_h", "otab_d", "yuv_stage", "draw_scratch"}
    assert snap["draw_scratch"] == pkg.ctx_mem_grow("draw_scratch", 1, 0, **geo) == [r for r in pkg.ctx_mem_plan(**geo)[0] if r["name"] == "xf"][0]["size"] * S + 256


def test_every_allocation_of_a_creation_may_fail(pkg, orc):
    w, h, fmt, slots = 40, 32, S420, (2, 3, 2, 4)
    L = pkg._mem_lib()
    rows, _ = pkg.ctx_mem_plan(w, h, fmt, 0, *slots)
    names = [r["name"] for r in rows]
    before = pkg.mem_outstanding()
    failed, ctx = [], None
    try:
        for n in range(1, 129):
            L.dsvg_debug_fail_alloc_at(n)
            rc, ctx = create(pkg, w, h, fmt, slots)
            if rc == 0:
                break
            text = L.dsvg_last_error().decode()
            assert rc == DSVG_ERR_HIP and not ctx.value and pkg.mem_outstanding() == before, (n, rc, text)
            assert text == "%s (%d bytes): out of memory" % (names[n - 1], rows[n - 1]["bytes"]), (n, text)
            failed.append(n)
        else:
            pytest.fail("no creation succeeded within 128 failing allocations")
    finally:
        L.dsvg_debug_fail_alloc_at(0)
    assert failed == list(range(1, len(rows) + 1))                            # every row once, each slab one allocation
    assert pkg.ctx_mem_live(ctx)["coef"] == rows[names.index("coef")]["bytes"]
    A.chk(pkg.lib(), pkg.lib().dsvg_ctx_sync(ctx))                            # (ends on hipGetLastError: nothing stale from the failures)
    pkg.lib().dsvg_ctx_destroy(ctx)
    assert pkg.mem_outstanding() == before
    clip = A.gen_clip(w, h, fmt, 0xC7D, 5, style=2)
    want, _ = A.orc_encode(clip, A.orc_cfg(w, h, fmt, qp=85, gop=12, rc_mode_cli=1))
    assert pkg.encode_clip(clip, w, h, fmt, qp=85, gop=12, rc_mode_cli=1) == want


def test_create_and_destroy_return_the_memory(pkg):
    """free device memory after 30 create / destroy cycles of the (16,16,16,32) context may not be lower by more than ONE such context:
    a thirtieth of it leaking per cycle would be"""
    w, h, fmt, slots = 96, 64, S420, (16, 16, 16, 32)
    _, tot = pkg.ctx_mem_plan(w, h, fmt, 0, *slots)
    rc, ctx = create(pkg, w, h, fmt, slots)                                   # (the runtime's own first-use allocations: not the cycles')
    A.chk(pkg.lib(), rc)
    pkg.lib().dsvg_ctx_destroy(ctx)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(30):
        rc, ctx = create(pkg, w, h, fmt, slots)
        A.chk(pkg.lib(), rc)
        pkg.lib().dsvg_ctx_destroy(ctx)
    free1 = torch.cuda.mem_get_info()[0]
    print("free before %d, after %d, one context %d" % (free0, free1, tot["device"]))
    assert free0 - free1 <= tot["device"]
