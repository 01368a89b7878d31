"""The plan of a coding call (csrc/dsvg_batch_plan.h) against the call that ran from it: 4 streams x 3 frame steps (I, P, P) with
ping-pong reconstruction slots and the vectors of dsvg_analyse, on a fused geometry and one that is not.  After dsvg_code_batch with
two coding streams the borders written (dsvg_recon_border of every kept slot) are the extents the device-free query
dsvg_code_batch_plan gives for the same jobs and context arguments, and the coded pictures are those of the same call on one stream."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A

pytestmark = pytest.mark.gpu

S, T = 4, 3


class PicOut(C.Structure):
    _fields_ = [("dc", C.c_int32 * 3), ("nruns", C.c_uint32 * 3), ("nbytes", C.c_uint32 * 3), ("payload", C.c_void_p * 3),
                ("rc_quant", C.c_int32), ("rc_pkt_len", C.c_uint32)]


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return m


def _code(pkg, w, h, clips, code_streams):
    """-> (coded planes per out slot, border extents per reconstruction slot, the query's plan of the call)"""
    L, fmt = pkg.lib(), A.SUBSAMP_420
    L.dsvg_ctx_create.argtypes = [C.POINTER(C.c_void_p)] + [C.c_int] * 9
    L.dsvg_load_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.dsvg_analyse.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]
    L.dsvg_code_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(pkg.PicJob)]
    L.dsvg_fetch_pictures.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(PicOut)]
    L.dsvg_recon_border.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.dsvg_ctx_destroy.argtypes = [C.c_void_p]
    n_src, n_recon, max_jobs, out_slots = T * S, 2 * S, S, T * S
    ctx = C.c_void_p(None)
    assert L.dsvg_ctx_create(C.byref(ctx), 0, w, h, fmt, 0, n_src, n_recon, max_jobs, out_slots) == 0, L.dsvg_last_error()
    try:
        L.dsvg_ctx_code_streams(ctx, code_streams)
        frames = np.ascontiguousarray(clips.transpose(1, 0, 2))               # source slot = t * S + s
        assert L.dsvg_load_frames(ctx, 0, T * S, frames.ctypes.data, 0, 1) == 0, L.dsvg_last_error()
        bw, bh, nbh, nbv = A.block_dims(w, h)
        nblk = nbh * nbv
        npairs = (T - 1) * S
        cur = (C.c_int * npairs)(*range(S, T * S))
        ref = (C.c_int * npairs)(*range(0, (T - 1) * S))
        mvs = np.zeros((npairs, nblk), dtype=A.MV_DTYPE)
        assert L.dsvg_analyse(ctx, npairs, cur, ref, mvs.ctypes.data) == 0, L.dsvg_last_error()
        stable = np.zeros((T * S, nblk), dtype=np.uint8)
        jobs = (pkg.PicJob * (T * S))()
        for t in range(T):
            for s in range(S):
                i = t * S + s
                # the stream's reconstructions alternate between slots s and S + s; the P pictures of the odd streams vouch that no later call
                # reads theirs: slot S + s gets what the last picture's vectors need, slot s nothing
                jobs[i] = pkg.PicJob(i, -1 if t == 0 else s + S * ((t + 1) % 2), s + S * (t % 2), 313, None if t == 0 else mvs[i - S].ctypes.data,
                                     stable[i].ctypes.data, i, 0, 0, (C.c_short * 4)(), int(t > 0 and s % 2 == 1))
        plan = pkg.code_batch_plan(w, h, fmt, n_recon, n_src, max_jobs, out_slots, code_streams, 0, T, S, jobs)
        assert L.dsvg_code_batch(ctx, T, S, jobs) == 0, L.dsvg_last_error()
        slots = (C.c_int * (T * S))(*range(T * S))
        outs = (PicOut * (T * S))()
        assert L.dsvg_fetch_pictures(ctx, T * S, slots, outs) == 0, L.dsvg_last_error()
        planes = [tuple((o.dc[p], o.nruns[p], C.string_at(o.payload[p], o.nbytes[p])) for p in range(3)) for o in outs]
        borders = np.zeros((n_recon, 8), dtype=np.int16)
        for r in range(n_recon):
            assert L.dsvg_recon_border(ctx, r, borders[r].ctypes.data) == 0, L.dsvg_last_error()
        return planes, borders, plan, bool((mvs["mode"] == 0).any())
    finally:
        L.dsvg_ctx_destroy(ctx)


@pytest.mark.parametrize("w,h,fused", [(96, 64, 1), (384, 240, 0)])
def test_the_call_runs_its_plan(pkg, w, h, fused):
    clips = np.stack([A.gen_clip(w, h, A.SUBSAMP_420, 0xBA7C + s, T, style=s % 3) for s in range(S)])
    planes2, borders, plan, inter = _code(pkg, w, h, clips, 2)
    assert plan["ng"] == 2 and plan["gk"] == (0, 2, 4) and plan["mc_fused"] == fused and inter
    # all jobs are I pictures first or P pictures only: device order is the caller's, and the last writer of slot r is the one in this table
    assert list(plan["order"]) == list(range(S)) * T
    last = {}
    for t in range(T):
        for s in range(S):
            last[s + S * (t % 2)] = t * S + s
    assert sorted(last) == list(range(2 * S))
    for r, d in last.items():
        assert borders[r].tolist() == plan["ext"][d].tolist(), (r, d)
    # (every kind of extent occurs: the whole border of a slot that outlives the call, nothing for a vouched picture nobody reads, and what
    # the vectors need -- at least 16 columns and 8 rows -- for a vouched one that the call's last step reads)
    assert all((borders[s] == 64).all() and (borders[S + s] == 64).all() for s in (0, 2))
    assert all((borders[s] == 0).all() and (borders[S + s] >= 8).all() for s in (1, 3))
    planes1, borders1, plan1, _ = _code(pkg, w, h, clips, 1)
    assert plan1["ng"] == 1 and (plan1["ext"] == plan["ext"]).all() and (borders1 == borders).all()
    assert planes2 == planes1, "two coding streams change the coded pictures"
