"""Every dispatch branch of the inverse transform of encoder and decoder pictures, on the GPU, against the oracle.

One geometry per class of tests/inv_plan.py (tests/inv_cases.py), three contents each.  Frame by frame, the encoder's inverse
kernels are counted (launches and algorithmic bytes per kernel: dsvg_prof_*) and must be the plan's -- which pins the branch each
geometry takes (er / eb, part4, the strips, the fused border) -- while every reconstruction and the stream must equal the
oracle's.  Then the clip in one call with two streams (more pictures per launch, the XCD tile remap), and the decoders on the
oracle's streams."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import inv_cases as IC
import inv_plan as P
from test_gpu_recon import border_mask, expected_raw
from test_gpu_stream import product_decode

pytestmark = pytest.mark.gpu

CONTENTS = list(IC.CONTENTS)


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    L = m.lib()
    assert L.dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    L.dsv1_batch_recon_slot.argtypes = [C.c_void_p, C.c_int]
    L.dsvg_download_recon_raw.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.dsvg_download_recon_asis.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.dsvg_recon_border.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return m


_oracle = {}


def oracle(g, content, qp_of=None):
    """(clip, stream, reconstructions) of the oracle encoder: content coded with the coding settings of `qp_of` (default: its own)"""
    key = (g, content, qp_of or content)
    if key not in _oracle:
        w, h, fmt = g
        clip = IC.make_content(w, h, fmt, content, 0x1A7 + 7 * w + h)
        stream, recs = A.orc_encode(clip, A.orc_cfg(w, h, fmt, **IC.cli(qp_of or content)), want_recon=True, eos=False)
        kinds = [p[5] & 1 for p in A.split_packets(stream) if p[5] & 4]
        assert kinds == [0] + [1] * (IC.NFRAMES - 1), "the case wants one I picture, then P pictures only: %s" % kinds
        _oracle[key] = (clip, stream, recs)
    return _oracle[key]


def check_recon(pkg, b, stream, g, want_planar, what):
    """the reconstruction the stream's last picture left: picture area + the border it vouches for as left, then the whole border"""
    L = pkg.lib()
    slot = L.dsv1_batch_recon_slot(b.h, stream)
    assert slot >= 0, what
    want = expected_raw(g[0], g[1], g[2], want_planar)
    got = np.zeros_like(want)
    ext = (C.c_short * 8)()
    assert L.dsvg_recon_border(b.ctx, slot, ext) == 0
    assert L.dsvg_download_recon_asis(b.ctx, slot, got.ctypes.data, got.size) == 0, L.dsvg_last_error()
    bad = np.nonzero((got != want) & border_mask(g[0], g[1], g[2], list(ext)))[0]
    assert bad.size == 0, "%s: %d reconstruction bytes differ (border %s), first at raw offset %d" % (what, bad.size, list(ext), int(bad[0]))
    assert L.dsvg_download_recon_raw(b.ctx, slot, got.ctypes.data, got.size) == 0, L.dsvg_last_error()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d bytes differ after the border was completed, first at raw offset %d" % (what, bad.size, int(bad[0]))


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("g", IC.GEOMETRIES, ids=IC.case_id)
def test_encoder_frame_by_frame(pkg, g, content):
    w, h, fmt = g
    plan = P.plan(w, h, fmt)
    clip, want_stream, want_rec = oracle(g, content)
    b = pkg.Batch(pkg.make_encoder_cfg(w, h, fmt, **IC.cli(content)), 1, 1)
    try:
        b.code_streams(1)
        inv = [k for k in b.kernel_names() if P.re_inverse.match(k)]
        assert set(inv) >= set(plan.p_kernels) | set(plan.i_kernels)
        b.tile_stats()
        got_stream, flagged = b"", 0
        for t in range(IC.NFRAMES):
            b.prof_enable(inv)
            got_stream += b.encode(clip[t].reshape(1, 1, -1))[0]
            st = b.tile_stats()
            want = plan.p_kernels if t else plan.i_kernels
            got = {}
            for k in inv:
                _, n, by = b.prof_get(k)
                if n:
                    got[k] = (n, by)
            where = "%s %s frame %d (%s)" % (IC.case_id(g), content, t, P.describe(plan.cls))
            assert got == want, "%s: inverse kernels (launches, bytes) %s, the plan says %s" % (where, got, want)
            if t:
                assert (st["fused_border_bytes"] > 0) == plan.chroma["fb"], "%s: %s" % (where, st)
                if content == "dense":
                    assert st["general_luma"] > 0, "%s: %s" % (where, st)
                    flagged += st["flagged_patches_luma"] + st["flagged_patches_chroma"]
            else:
                assert st["fused_border_bytes"] == 0, "%s: %s" % (where, st)
            check_recon(pkg, b, 0, g, want_rec[t], where)
        b.prof_enable([])
        # patches whose level-1 symbols were fetched: where the fast luma tiles or the chroma patch kernel run (on planes that
        # take neither, these small pictures have none)
        if content == "dense" and (plan.luma["kind"] == "fast" or P.KPATCH_C in plan.p_kernels):
            assert flagged > 0, "%s dense: no flagged patches in the P pictures" % IC.case_id(g)
        assert got_stream == want_stream, "%s %s: stream differs from the oracle's" % (IC.case_id(g), content)
    finally:
        b.close()


@pytest.mark.parametrize("g", IC.GEOMETRIES, ids=IC.case_id)
def test_encoder_batched(pkg, g):
    """the whole clip in one call, two streams of different content (coded alike), the default coding streams"""
    w, h, fmt = g
    runs = [oracle(g, c, "sparse") for c in ("dense", "sparse")]
    b = pkg.Batch(pkg.make_encoder_cfg(w, h, fmt, **IC.cli("sparse")), 2, IC.NFRAMES)
    try:
        got = b.encode(np.stack([r[0] for r in runs]))
        for s, (_, want_stream, want_rec) in enumerate(runs):
            assert got[s] == want_stream, "%s stream %d differs from the oracle's" % (IC.case_id(g), s)
            check_recon(pkg, b, s, g, want_rec[-1], "%s stream %d last picture" % (IC.case_id(g), s))
    finally:
        b.close()


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("g", IC.GEOMETRIES, ids=IC.case_id)
def test_decoders(pkg, g, content):
    """dsv_dec and the batched decoder (host and device output) on the oracle's stream: the oracle decoder's frames, which are
    the oracle encoder's reconstructions where the scan regions do not overlap"""
    w, h, fmt = g
    _, stream, recs = oracle(g, content)
    want = A.orc_decode(stream, w, h, fmt)
    assert len(want) == IC.NFRAMES
    if not P.scan_overlap(w, h, fmt):
        for t in range(IC.NFRAMES):
            A.assert_same("%s %s oracle decode == recon %d" % (IC.case_id(g), content, t), want[t], recs[t])
    got = product_decode(pkg, stream)
    assert len(got) == IC.NFRAMES
    for t in range(IC.NFRAMES):
        A.assert_same("%s %s dsv_dec frame %d" % (IC.case_id(g), content, t), got[t], want[t])
    pk = A.split_packets(stream)
    for on_device in (False, True):
        d = pkg.DecBatch(w, h, fmt, 1)
        try:
            frames = []
            for p in pk:
                if on_device:
                    _, status, _ = d.decode([p], on_device=True)
                    out = d.download()
                else:
                    out, status, _ = d.decode([p])
                if p[5] & 4:
                    assert status[0] == 0
                    frames.append(out[0].copy())
        finally:
            d.close()
        assert len(frames) == IC.NFRAMES
        for t in range(IC.NFRAMES):
            A.assert_same("%s %s DecBatch(device=%d) frame %d" % (IC.case_id(g), content, on_device, t), frames[t], want[t])
