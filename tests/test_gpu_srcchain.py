"""The source side of a session on the device against its plan (csrc/host/dsv1_srcchain_plan.h through dsv1_srcchain_plan_set / _call).
One scripted walk of setter, reset and seek calls on a Batch and one on a ResLadder: after every call the return code is the plan's,
the session's source_input accessor is the planned state's, and the batch's lane exists exactly when the plan says so.  Each walk
produces every refusal row its session's functions can reach (a ladder has no format, orientation or reframe setter), the two rows on
frames_per_call in a second session of 3 frames per call, which 64x48 4:2:0 x 2 sources x 4 frames cannot refuse.  Then one call
through convert + levels + denoise + overlays in the three clip forms equals the packets of the same batch fed the numpy-transformed
clip, and a call whose overlays are not active is the bypass: nothing enqueued, the bytes of no overlay at all."""
import collections
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import _denoise as D
import _levels as LV
import _overlay as OV
import _pixfmt as PF

pytestmark = pytest.mark.gpu

ERR_ARG = -2
W, H, FMT, S, F = 64, 48, A.SUBSAMP_420, 2, 4
IN_W, IN_H = 80, 60
CRF = dict(gop=4, rc_mode_cli=1, scd=1, qp=80)
T_GRADE = LV.compose(LV.range_(1, 0), LV.adjust(24, 228, 16, 235, 300))
DN = (24, 24)


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return m


def po(pkg, o):
    return pkg.Overlay(o["planes"], o["w"], o["h"], o["x"], o["y"], o["source"], o["t0"], o["dur"], o["fade_in"], o["fade_out"], o["opacity"], o["reserved"])


def logo(t0=0):
    return OV.ov(OV.bitmap(16, 9, FMT, 41), 16, 9, x=W - 22, y=4, source=-1, t0=t0, opacity=200)


# ---- the walks ---------------------------------------------------------------------------------------------------------------------
class Walk:
    """a session, the plan's state of its chain, and the rows of the refusal table produced so far"""

    def __init__(self, pkg, sess, prefix, keep_lane, frames):
        self.pkg, self.sess, self.prefix, self.rows = pkg, sess, prefix, collections.Counter()
        self.state = pkg.SrcChainState(nsrc=S, F=frames, subsamp=FMT, keep_lane=keep_lane, ow=W, oh=H)
        self.geom = pkg.srcchain_plan_set(self.state, pkg.SrcChainReq(op=pkg.SC_OP_SET, kind=pkg.SC_DENOISE, valid=1)).g
        self.check("open")

    def check(self, what):
        s, g = self.sess, self.geom
        assert (s.in_frames, s.frame_bytes, s.in_dims) == (g.frames_in, g.frame_in_bytes, (g.w, g.h)), what
        if self.prefix == "dsv1_batch_":
            assert bool(s.L.dsv1_batch_has_source_lane(s.h)) == bool(g.lane), what

    def call(self, fn, req, *args, busy=0):
        """the session's function `fn` with args, and the plan's answer to `req`"""
        req.busy = busy
        rc = getattr(self.sess.L, self.prefix + fn)(self.sess.h, *args)
        try:
            plan = self.pkg.srcchain_plan_set(self.state, req)
            want = 0
            self.state, self.geom = plan.next, plan.g
        except self.pkg.SrcChainRefused as e:
            want = e.rc
            self.rows[e.row] += 1
        assert rc == want, (fn, rc, want)
        self.check(fn)
        return rc

    def set(self, fn, kind, arg, busy=0, **numbers):
        numbers.setdefault("set", int(arg is not None))
        numbers.setdefault("valid", 1)
        req = self.pkg.SrcChainReq(op=self.pkg.SC_OP_SET, kind=kind, **numbers)
        return self.call(fn, req, *(arg if isinstance(arg, tuple) else (None if arg is None else C.byref(arg),)), busy=busy)

    def reset(self, fn, kind, source, busy=0):
        return self.call(fn, self.pkg.SrcChainReq(op=self.pkg.SC_OP_RESET, kind=kind, source=source), source, busy=busy)

    def seek(self, fn, source, t):
        return self.call(fn, self.pkg.SrcChainReq(op=self.pkg.SC_OP_SEEK, kind=self.pkg.SC_OVERLAY, source=source), source, C.c_int64(t))

    def produced(self, texts, words):
        missing = [w for w in words if not any(w in texts[r] for r in self.rows)]
        assert not missing, (missing, dict(self.rows))


def temporal_steps(k, p, deint, ivtc, dreset, ireset):
    """the deinterlacer and the inverse telecine, the two occupants of one position, with their resets: as a batch and a ladder name them"""
    pkg = k.pkg
    k.set(deint, pkg.SC_DEINTERLACE, pkg.Deint(7, 1), valid=0, mode=7)                  # no such mode
    k.set(deint, pkg.SC_DEINTERLACE, pkg.Deint(pkg.DEINT_FIELD, 1), mode=pkg.DEINT_FIELD)
    assert k.sess.in_frames == F // 2
    k.set(ivtc, pkg.SC_IVTC, pkg.Ivtc(1, 0))                                            # refused: a deinterlacer is set
    k.set(ivtc, pkg.SC_IVTC, None)                                                      # taken, untouched
    k.reset(dreset, pkg.SC_DEINTERLACE, S)                                              # no such source
    k.reset(ireset, pkg.SC_IVTC, -1)                                                    # not set
    assert k.reset(dreset, pkg.SC_DEINTERLACE, -1) == 0
    k.set(deint, pkg.SC_DEINTERLACE, None)
    k.set(ivtc, pkg.SC_IVTC, pkg.Ivtc(1, 300), valid=0)                                 # no such threshold
    assert k.set(ivtc, pkg.SC_IVTC, pkg.Ivtc(1, 0)) == 0
    assert k.sess.in_frames == F // 4 * 5
    k.set(deint, pkg.SC_DEINTERLACE, pkg.Deint(pkg.DEINT_FRAME, 1), mode=pkg.DEINT_FRAME)    # refused: an inverse telecine is set
    k.set(deint, pkg.SC_DEINTERLACE, None)                                              # taken, untouched
    assert k.reset(ireset, pkg.SC_IVTC, 0) == 0
    k.set(p + "denoise", pkg.SC_DENOISE, pkg.Denoise(0, 0), valid=0)                    # no strength at all
    assert k.set(p + "denoise", pkg.SC_DENOISE, pkg.Denoise(*DN)) == 0


def overlay_steps(k, p, seek):
    pkg = k.pkg
    off = OV.ov(OV.bitmap(16, 9, FMT, 41), 16, 9, x=W - 8, y=4)                         # hangs over the canvas
    for o, valid in ((off, 0), (logo(), 1)):
        arr = (pkg.Overlay * 1)(po(pkg, o))
        k.set(p + "overlays", pkg.SC_OVERLAY, (arr, 1), valid=valid)
    k.seek(seek, S, 7)                                                                  # no such source
    assert k.seek(seek, -1, 7) == 0


def odd_frames_steps(k, deint, ivtc):
    """a session of 3 frames per call: the two rules on frames_per_call"""
    pkg = k.pkg
    assert k.set(deint, pkg.SC_DEINTERLACE, pkg.Deint(pkg.DEINT_FIELD, 1), mode=pkg.DEINT_FIELD) == ERR_ARG
    assert k.set(ivtc, pkg.SC_IVTC, pkg.Ivtc(1, 0)) == ERR_ARG
    assert k.set(deint, pkg.SC_DEINTERLACE, pkg.Deint(pkg.DEINT_FRAME, 1), mode=pkg.DEINT_FRAME) == 0


ALL_WORDS = ["no such source", "even frames_per_call", "multiple of 4", "in flight", "not set", "a deinterlacer while", "an inverse telecine while",
             "not a deinterlacer", "not an inverse telecine", "not a noise filter", "not a valid list of overlays"]
BATCH_WORDS = ["a reframe while a source format", "a reframe while an orientation", "an orientation while a source format",
               "not a valid pixel or RGB format", "not an orientation", "not a valid reframe"]


def test_setter_walk_on_a_batch(pkg):
    texts = pkg.srcchain_plan_texts()
    cfg = pkg.make_encoder_cfg(W, H, FMT, **CRF)
    b = pkg.Batch(cfg, S, F)
    try:
        k = Walk(pkg, b, "dsv1_batch_", 0, F)
        assert not b.L.dsv1_batch_has_source_lane(b.h)
        rf = pkg.Reframe(IN_W, IN_H, (8, 6, W, H), (W, H))
        small = pkg.Reframe(IN_W, IN_H, (8, 6, W // 2, H // 2), (W // 2, H // 2))
        dims = lambda r: dict(w=r.in_w, h=r.in_h, out_w=r.out_w, out_h=r.out_h)
        k.set("set_source_reframe", pkg.SC_REFRAME, small, **dims(small))               # onto another canvas
        assert k.set("set_source_reframe", pkg.SC_REFRAME, rf, **dims(rf)) == 0
        k.set("set_source_orient", pkg.SC_ORIENT, (9,), mode=9)                         # no such code
        assert k.set("set_source_orient", pkg.SC_ORIENT, (pkg.Orient.ROT90,), mode=pkg.Orient.ROT90) == 0
        assert b.in_dims == (IN_H, IN_W)
        k.set("set_source_reframe", pkg.SC_REFRAME, None)                               # refused: an orientation is set
        nv12 = pkg.PixFormat(pkg.PIX_SEMIPLANAR_UV)
        fb = pkg.pix_frame_bytes(nv12, IN_H, IN_W, FMT)
        k.set("set_source_format", pkg.SC_CONVERT, pkg.PixFormat(99), valid=0)          # no such layout
        assert k.set("set_source_format", pkg.SC_CONVERT, nv12, frame_bytes=fb) == 0
        k.set("set_source_orient", pkg.SC_ORIENT, (0,), mode=0)                         # refused: a format is set
        k.set("set_source_reframe", pkg.SC_REFRAME, None)                               # refused: a format is set
        lv = pkg.Levels.from_tables(T_GRADE)
        assert k.set("set_source_levels", pkg.SC_LEVELS, lv) == 0
        assert k.set("set_source_levels", pkg.SC_LEVELS, pkg.Levels.identity(), identity=1) == 0    # the identity clears
        assert k.state.kind[1] == pkg.SC_NONE
        assert k.set("set_source_levels", pkg.SC_LEVELS, lv) == 0
        temporal_steps(k, "set_source_", "set_source_deinterlace", "set_source_ivtc", "deinterlace_reset", "ivtc_reset")
        overlay_steps(k, "set_source_", "overlay_seek")
        # busy: one submit in flight, collected before the walk goes on
        b.submit(np.zeros((S, b.in_frames, b.frame_bytes), dtype=np.uint8))
        assert k.set("set_source_denoise", pkg.SC_DENOISE, None, busy=1) == ERR_ARG
        assert k.reset("denoise_reset", pkg.SC_DENOISE, -1, busy=1) == ERR_ARG
        b.collect()
        assert k.reset("denoise_reset", pkg.SC_DENOISE, -1) == 0
        # back to nothing, in an order the rules take: the lane goes with the last pass
        for fn, kind, arg, nums in (("set_source_overlays", pkg.SC_OVERLAY, (None, 0), {"set": 0}), ("set_source_denoise", pkg.SC_DENOISE, None, {}),
                                    ("set_source_ivtc", pkg.SC_IVTC, None, {}), ("set_source_levels", pkg.SC_LEVELS, None, {}),
                                    ("set_source_format", pkg.SC_CONVERT, None, {}), ("set_source_orient", pkg.SC_ORIENT, (0,), {}),
                                    ("set_source_reframe", pkg.SC_REFRAME, None, {})):
            assert b.L.dsv1_batch_has_source_lane(b.h)
            assert k.set(fn, kind, arg, **nums) == 0
        assert not b.L.dsv1_batch_has_source_lane(b.h) and (b.in_frames, b.in_dims) == (F, (W, H))
    finally:
        b.close()
    b3 = pkg.Batch(cfg, S, 3)
    try:
        k3 = Walk(pkg, b3, "dsv1_batch_", 0, 3)
        odd_frames_steps(k3, "set_source_deinterlace", "set_source_ivtc")
    finally:
        b3.close()
    k.rows.update(k3.rows)
    k.produced(texts, ALL_WORDS + BATCH_WORDS)
    assert len(k.rows) == len([t for t in texts if t]), "a row of the table this walk never produced"


def test_setter_walk_on_a_resolution_ladder(pkg):
    texts = pkg.srcchain_plan_texts()
    geoms = [(W, H, [pkg.make_encoder_cfg(W, H, FMT, **CRF)])]
    r = pkg.ResLadder(W, H, FMT, geoms, S, F)
    try:
        k = Walk(pkg, r, "dsv1_resladder_", 1, F)
        temporal_steps(k, "set_", "set_deinterlace", "set_ivtc", "deinterlace_reset", "ivtc_reset")
        overlay_steps(k, "set_", "overlay_seek")
        r.submit(np.zeros((S, r.in_frames, r.frame_bytes), dtype=np.uint8))
        assert k.set("set_levels", pkg.SC_LEVELS, pkg.Levels.from_tables(T_GRADE), busy=1) == ERR_ARG
        assert k.reset("ivtc_reset", pkg.SC_IVTC, -1, busy=1) == ERR_ARG
        r.collect()
        assert k.set("set_levels", pkg.SC_LEVELS, pkg.Levels.from_tables(T_GRADE)) == 0
        assert k.set("set_overlays", pkg.SC_OVERLAY, (None, 0), set=0) == 0
        for fn, kind in (("set_denoise", pkg.SC_DENOISE), ("set_ivtc", pkg.SC_IVTC), ("set_levels", pkg.SC_LEVELS)):
            assert k.set(fn, kind, None) == 0
        assert (r.in_frames, r.in_dims, r.frame_bytes) == (F, (W, H), A.frame_bytes(W, H, FMT))
    finally:
        r.close()
    r3 = pkg.ResLadder(W, H, FMT, geoms, S, 3)
    try:
        k3 = Walk(pkg, r3, "dsv1_resladder_", 1, 3)
        odd_frames_steps(k3, "set_deinterlace", "set_ivtc")
    finally:
        r3.close()
    k.rows.update(k3.rows)
    k.produced(texts, ALL_WORDS)


# ---- one call in the three clip forms ------------------------------------------------------------------------------------------------
def encode_call(b, call, form):
    """submit / collect one call -> the streams' packets; a caller's device clip must come back unchanged"""
    if form == "host":
        b.submit(call)
        return [bytes(x) for x in b.collect()]
    p = b.upload(call)
    b.submit(p, on_device=True, held=form == "held")
    if form == "held":
        got = [bytes(x) for x in b.collect()]
    back = np.zeros(call.size, dtype=np.uint8)
    b.sync()
    assert b.L.dsvg_dev_download(b.ctx, back.ctypes.data, p, back.size) == 0
    assert np.array_equal(back, call.reshape(-1)), "the caller's device clip was written (%s)" % form
    return got if form == "held" else [bytes(x) for x in b.collect()]


@pytest.fixture(scope="module")
def clips(pkg):
    """the planar sources, their NV12 packing, what the chain must make of them, and the packets of a batch fed that"""
    f = PF.pf(PF.SEMI_UV)
    planar = [A.gen_clip(W, H, FMT, 0x5C0 + s, F, style=s & 1) for s in range(S)]
    raws = [PF.pack(c.astype(np.uint32), f, W, H, FMT, np.random.default_rng(s)).reshape(F, -1) for s, c in enumerate(planar)]
    made = []
    for s, r in enumerate(raws):
        x = PF.convert(r.reshape(-1), f, W, H, FMT, F)
        assert np.array_equal(x, planar[s])
        x = D.denoise_clip(LV.levels_clip(x, W, H, FMT, T_GRADE), W, H, FMT, *DN)[0]
        made.append(OV.composite(x, W, H, FMT, [logo()], 0, s))
    cfg = pkg.make_encoder_cfg(W, H, FMT, **CRF)
    fed = {}
    for name, cl in (("made", made), ("planar", planar)):
        b = pkg.Batch(cfg, S, F)
        try:
            fed[name] = encode_call(b, np.stack(cl), "host")
        finally:
            b.close()
    assert fed["made"] != fed["planar"]
    return dict(cfg=cfg, planar=np.stack(planar), raws=np.ascontiguousarray(np.stack(raws)), fed=fed)


@pytest.mark.parametrize("form", ["host", "device", "held"])
def test_convert_levels_denoise_overlays_in_one_call(pkg, clips, form):
    b = pkg.Batch(clips["cfg"], S, F)
    try:
        b.set_source_format(pkg.PixFormat(pkg.PIX_SEMIPLANAR_UV))
        b.set_source_levels(pkg.Levels.from_tables(T_GRADE))
        b.set_source_denoise(pkg.Denoise(*DN))
        b.set_source_overlays([po(pkg, logo())])
        assert b.frame_bytes == clips["raws"].shape[2]
        got = encode_call(b, clips["raws"], form)
    finally:
        b.close()
    assert got == clips["fed"]["made"], form


def test_overlays_not_active_on_a_held_clip_is_the_bypass(pkg, clips):
    state = pkg.SrcChainState(nsrc=S, F=F, subsamp=FMT, keep_lane=0, ow=W, oh=H)
    state.kind[6] = pkg.SC_OVERLAY
    plan = pkg.srcchain_plan_call(state, 2, False)
    assert plan.bypass and plan.nsteps == 0 and plan.upload == 0 and plan.out == pkg.SC_CALLER and plan.advance == F
    b = pkg.Batch(clips["cfg"], S, F)
    try:
        b.set_source_overlays([po(pkg, logo(t0=100))])                # (first shown long after this call)
        assert b.L.dsv1_batch_has_source_lane(b.h)
        got = encode_call(b, clips["planar"], "held")
    finally:
        b.close()
    assert got == clips["fed"]["planar"]
