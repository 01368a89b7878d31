"""The decoder call behind its plan (csrc/dsvg_dec_plan.h), on the GPU: dsvg_decode_pictures on contexts of the test's own, with jobs
built from the packets of a short clip the project's encoder coded (tests/dec_cases.py: packet_job).

  * the launches the kernel profiler counts -- k_hz_scatter_lv, and the k_mc bracket that holds k_mc and the k_mc_patch pair -- are what
    dsvg_decode_plan says for the same jobs and context arguments, and the pictures are the oracle's;
  * the same call unprofiled, where the motion compensation forks to the second stream, gives the same pictures;
  * a refused call changes nothing: the pictures of the calls around it are those of a context that never saw it -- plain, with the
    debug overlay read after the refusal, and with a flagged picture whose pending record has to outlive the refusal."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A
import dec_cases as K
from _hzbits import plane_payload, region_base, splice

pytestmark = pytest.mark.gpu

S = 4                                       # streams = pictures per call
MAX_JOBS = 16                               # a context with a second coding stream
N_RECON = 3 * MAX_JOBS


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    L = m.lib()
    assert L.dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    L.dsvg_ctx_create.argtypes = [C.POINTER(C.c_void_p)] + [C.c_int] * 9
    L.dsvg_ctx_destroy.argtypes = [C.c_void_p]
    L.dsvg_ctx_destroy.restype = None
    L.dsvg_decode_pictures.argtypes = [C.c_void_p, C.c_int, C.POINTER(m.DecJob)]
    L.dsvg_download_recon.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.dsvg_ctx_draw_info.argtypes = [C.c_void_p, C.c_int]
    L.dsvg_ctx_decoder_redone.restype = C.c_long
    L.dsvg_ctx_decoder_redone.argtypes = [C.c_void_p]
    return m


_streams = {}


def stream_of(pkg, geom):
    """(picture packets I P P of the geometry's clip, the oracle's three frames)"""
    if geom not in _streams:
        w, h, fmt = K.GEOMS[geom]
        clip = A.gen_clip(w, h, fmt, 0xDEC0DE, 3, style=1)
        stream = pkg.encode_clip(clip, w, h, fmt, qp=85, gop=12, rc_mode_cli=1)
        pics = [p for p in A.split_packets(stream) if p[5] & 4]
        assert [p[5] & 1 for p in pics] == [0, 1, 1]
        _streams[geom] = (pics, A.orc_decode(stream, w, h, fmt))
    return _streams[geom]


class Ctx:
    def __init__(self, pkg, geom):
        self.pkg, self.L, self.geom = pkg, pkg.lib(), geom
        self.w, self.h, self.fmt = K.GEOMS[geom]
        self.h_ = C.c_void_p(None)
        A.chk(self.L, self.L.dsvg_ctx_create(C.byref(self.h_), 0, self.w, self.h, self.fmt, 1, 1, N_RECON, MAX_JOBS, MAX_JOBS))
        names = [self.L.dsvg_prof_kernel_name(i).decode() for i in range(self.L.dsvg_prof_kernels())]
        self.kid = {k: names.index(k) for k in ("k_hz_scatter_lv", "k_mc")}

    def call(self, jobs):
        return K.Call.of_jobs(self.geom, jobs, MAX_JOBS, N_RECON)

    def decode(self, jobs):
        return self.L.dsvg_decode_pictures(self.h_, len(jobs), self.call(jobs).c_jobs())

    def frame(self, slot):
        out = np.zeros(A.frame_bytes(self.w, self.h, self.fmt), dtype=np.uint8)
        A.chk(self.L, self.L.dsvg_download_recon(self.h_, slot, out.ctypes.data))
        return out

    def launches(self, name):
        ms, n, by = C.c_double(0), C.c_long(0), C.c_double(0)
        A.chk(self.L, self.L.dsvg_prof_get(self.h_, self.kid[name], C.byref(ms), C.byref(n), C.byref(by)))
        return n.value

    def close(self):
        if self.h_:
            self.L.dsvg_ctx_destroy(self.h_)
            self.h_ = None


def warm_up(pics, w, h):
    """the I pictures of streams 1 .. 3 into their slots"""
    return [K.packet_job(pics[0], w, h, -1, s) for s in range(1, S)]


def call_a(pics, w, h, first=None):
    """one I picture (stream 0 starts) and three P pictures, the I picture second in the caller's order"""
    p1 = pics[1] if first is None else first
    jobs = [K.packet_job(p1 if s == 1 else pics[1], w, h, s, MAX_JOBS + s) for s in range(1, S)]
    jobs.insert(1, K.packet_job(pics[0], w, h, -1, 0))
    return jobs                                                 # frames: slot 0 = frame 0; slots MAX_JOBS + 1 .. 3 = frame 1


def call_b(pics, w, h):
    """four P pictures that predict from call A's"""
    return [K.packet_job(pics[1], w, h, 0, MAX_JOBS)] + [K.packet_job(pics[2], w, h, MAX_JOBS + s, s) for s in range(1, S)]


@pytest.mark.parametrize("geom", ["96x64", "384x240"])
def test_launches_are_the_plans_and_the_fork_changes_nothing(pkg, orc, geom):
    w, h, fmt = K.GEOMS[geom]
    pics, want = stream_of(pkg, geom)
    got = {}
    for profiled in (True, False):
        c = Ctx(pkg, geom)
        try:
            L = c.L
            A.chk(L, c.decode(warm_up(pics, w, h)))
            jobs = call_a(pics, w, h)
            plan = c.call(jobs).plan(pkg.DEC_PROFILED if profiled else 0)
            assert plan["nI"] == 1 and list(plan["order"]) == [1, 0, 2, 3]
            assert plan["fork"] == (0 if profiled else 1) and plan["second_stream"] == 1
            assert plan["mc"] == (2 if geom == "96x64" else 1)
            if profiled:
                A.chk(L, L.dsvg_prof_enable(c.h_, (1 << c.kid["k_hz_scatter_lv"]) | (1 << c.kid["k_mc"])))
                A.chk(L, L.dsvg_prof_reset(c.h_))
            A.chk(L, c.decode(jobs))
            frames = [c.frame(0)] + [c.frame(MAX_JOBS + s) for s in range(1, S)]
            assert L.dsvg_ctx_decoder_redone(c.h_) == 0
            if profiled:
                assert c.launches("k_hz_scatter_lv") == (1 if plan["scatter_one"] else 3)
                # the k_mc bracket: the whole-picture launch, or the listed blocks (where there are any) and the k_mc_patch pair
                assert c.launches("k_mc") == (1 if plan["mc"] == 1 else 1 + (plan["iln"] > 0))
                A.assert_same("%s: I picture" % geom, frames[0], want[0])
                for s in range(1, S):
                    A.assert_same("%s: P picture of stream %d" % (geom, s), frames[s], want[1])
            got[profiled] = frames
        finally:
            c.close()
    for s in range(S):
        A.assert_same("%s: picture %d with the fork against the profiled run" % (geom, s), got[False][s], got[True][s])


def flagged_p_picture(pics, w, h):
    """the clip's first P picture with a luma plane whose symbol of 40000 the int16 symbol planes cannot hold: its call is decoded again"""
    b2, sw2 = region_base(w, h, 2, 1)
    b1, sw1 = region_base(w, h, 1, 2)
    entries = sorted([(5, 3), (b1 + 4 * sw1 + 9, -2), (b2 + 10 * sw2 + 10, 40000), (b2 + 30 * sw2 + 20, 1)])
    return splice(pics[1], {0: plane_payload(7, entries)})


@pytest.mark.parametrize("how", ["plain", "draw_info", "flagged"])
def test_a_refused_call_changes_nothing(pkg, orc, how):
    geom = "96x64"
    w, h, fmt = K.GEOMS[geom]
    pics, want = stream_of(pkg, geom)
    first = flagged_p_picture(pics, w, h) if how == "flagged" else None
    out = {}
    for refuse in (False, True):
        c = Ctx(pkg, geom)
        try:
            L = c.L
            if how == "draw_info":
                A.chk(L, L.dsvg_ctx_draw_info(c.h_, 7))
            A.chk(L, c.decode(warm_up(pics, w, h)))
            A.chk(L, c.decode(call_a(pics, w, h, first)))
            if refuse:
                bad = call_b(pics, w, h)
                bad[1]["recon"] = N_RECON                        # the second job in the caller's order: a slot out of range
                assert c.decode(bad) == -2 and L.dsvg_last_error().decode() == "bad decode job 1"
                bad = call_b(pics, w, h)
                bad[2]["lens"][1] = A.coef_dims(w, h, fmt, 1)[0] * A.coef_dims(w, h, fmt, 1)[1] * 8 + 1
                assert c.decode(bad) == -2 and L.dsvg_last_error().decode() == "plane 1 of decode job 2: bad length"
                assert L.dsvg_ctx_decoder_redone(c.h_) == 0      # (the refused calls did not settle call A either)
            fa = [c.frame(0)] + [c.frame(MAX_JOBS + s) for s in range(1, S)] if how == "draw_info" else None
            A.chk(L, c.decode(call_b(pics, w, h)))
            fb = [c.frame(MAX_JOBS)] + [c.frame(s) for s in range(1, S)]
            if fa is None:                                       # (read behind call B, so that call A is still pending when B arrives)
                fa = [c.frame(0)] + [c.frame(MAX_JOBS + s) for s in range(1, S)]
            assert L.dsvg_ctx_decoder_redone(c.h_) == (1 if how == "flagged" else 0)
            out[refuse] = fa + fb
        finally:
            c.close()
    for i, (a, b) in enumerate(zip(out[True], out[False])):
        A.assert_same("%s: download %d after the refused calls against a context that never saw them" % (how, i), a, b)
    if how == "plain":
        A.assert_same("call A's I picture", out[True][0], want[0])
        A.assert_same("call B's picture of stream 0", out[True][S], want[1])
        A.assert_same("call B's picture of stream 2", out[True][S + 2], want[2])
