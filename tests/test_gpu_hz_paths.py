"""Every collect, scan and emit branch of the entropy pack stage (csrc/k_hzcc.hip), on the GPU, against the oracle.

tests/hz_plan.py models the stage's branches, tests/hz_cases.py lists the cases and tests/test_hz_plan_host.py proves on the CPU
that they reach every label.  Here the cases run on the device: the operator seam (k_hz_quant<false>, every chunk unpacked) on
built coefficient planes, the pipeline frame by frame (collect, the packed chunks, the list kernels; the entropy kernels launched
per step must be the model's), one step with an I and a P job, the LL quantiser and the list kernels switched off, and 33 streams
of 2048x2080 for the second tile of the 256-thread scan.  Where bytes differ the message names, through the model, the plane, the
first differing chunk, its rounds and its labels."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import _cabi as A
import hz_cases as HC
import hz_plan as H
from test_gpu_inv_paths import check_recon

pytestmark = pytest.mark.gpu

OP = HC.op_cases()


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


@pytest.fixture(scope="module")
def prod():
    L = A.load_prod()
    assert L.dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return L


def plane_diff(model, rec, got, want, what):
    """got / want: the bit streams the plane was written to (rec['at'] is its payload's offset in `want`)"""
    n = (rec["bits"] + 7) // 8
    return "%s (%dx%d, ll_end %d, %d chunks): %s" % (what, model.w, model.h, model.ll_end, model.nchunks,
                                                      model.explain(bytes(got[rec["at"]:rec["at"] + n]), bytes(want[rec["at"]:rec["at"] + n])))


@pytest.mark.parametrize("name", list(OP))
def test_operator_case(prod, orc, name):
    w, h, co, labels = OP[name]
    model, want, want_co, rec = HC.op_plane(w, h, co)
    assert set(labels) <= model.labels
    got, got_co = HC.op_encode(prod, "dsvg_op_encode_plane", w, h, co)
    assert got == want, "%s: packed plane differs (%d vs %d bytes): %s" % (name, len(got), len(want), plane_diff(model, rec, got, want, "plane"))
    A.assert_same("%s: dequantised coefficients" % name, got_co, want_co, (h, w))


def stream_diff(got, want, pictures, seam="pipe", njobs=1):
    """where a stream first differs from the oracle's, in the model's words"""
    n = min(len(got), len(want))
    first = next((i for i in range(n) if got[i] != want[i]), n)
    msg = "stream differs from the oracle's, first at byte %d (%d vs %d bytes)" % (first, len(got), len(want))
    o = 0
    for k, p in enumerate(A.split_packets(want)):
        if o <= first < o + len(p):
            for t, pic in enumerate(pictures):
                if pic["packet"] != k:
                    continue
                for rec in pic["planes"]:
                    if rec["at"] <= first - o < rec["at"] + (rec["bits"] + 7) // 8 + 1:
                        return msg + "; " + plane_diff(HC.model_of(rec, seam, njobs), rec, got[o:o + len(p)], p, "picture %d (%s) plane %d" % (t, pic["kind"], rec["cur_plane"]))
                return msg + "; picture %d (%s), outside the planes' payloads (packet byte %d)" % (t, pic["kind"], first - o)
        o += len(p)
    return msg


def run_frame_by_frame(pkg, g, clips, runs, cfg_kw, what, llq=True, list_pack=True, recon=True):
    """clips [stream][frame] coded one frame step at a time on one coding stream: per step the entropy kernels launched are the
    model's, every reconstruction the oracle's; then every stream.  runs: pipe_oracle's tuple per stream"""
    w, h, fmt = g
    S, n = len(clips), clips[0].shape[0]
    b = pkg.Batch(pkg.make_encoder_cfg(w, h, fmt, **cfg_kw), S, 1)
    try:
        b.code_streams(1)
        watched = [k for k in H.ENTROPY_KERNELS if k in b.kernel_names()]
        assert watched == H.ENTROPY_KERNELS, set(H.ENTROPY_KERNELS) - set(watched)
        got = [b""] * S
        for t in range(n):
            b.prof_enable(watched)
            out = b.encode(np.stack([c[t:t + 1] for c in clips]))
            kinds = [r[3][t]["kind"] for r in runs]
            want = H.step_kernels(kinds, llq, list_pack)
            launched = {k: b.prof_get(k)[1] for k in watched if b.prof_get(k)[1]}
            assert launched == want, "%s frame %d (%s): entropy kernels launched %s, the model says %s" % (what, t, "".join(kinds), launched, want)
            assert pkg.dispatch_last()["threads"][1] == H.scan_threads(S), "%s frame %d: %s" % (what, t, pkg.dispatch_last())
            for s in range(S):
                got[s] += bytes(out[s])
                if recon:
                    check_recon(pkg, b, s, g, runs[s][2][t], "%s frame %d stream %d" % (what, t, s))
        b.prof_enable([])
        for s in range(S):
            assert got[s] == runs[s][1], "%s stream %d: %s" % (what, s, stream_diff(got[s], runs[s][1], runs[s][3], njobs=S))
    finally:
        b.close()


@pytest.mark.parametrize("name", [c[0] for c in HC.PIPE_CASES])
def test_pipeline_case(pkg, name):
    _, g, content, qp, n, labels = HC.pipe_case(name)
    run = HC.pipe_oracle(name)
    run_frame_by_frame(pkg, g, [run[0]], [run], dict(HC.CODING, qp=qp), name)


def test_one_step_with_an_i_and_a_p_job(pkg):
    """two streams, the second with a scene cut: launch_hz_pack with ndense > 0 and nsparse > 0"""
    runs = HC.cut_oracle()
    assert [[p["kind"] for p in r[3]] for r in runs] == [["I", "P", "P"], ["I", "I", "P"]]
    run_frame_by_frame(pkg, HC.CUT_G, [r[0] for r in runs], runs, dict(HC.CUT_CODING, qp=HC.CUT_QP), "scene cut")


@pytest.fixture
def switch():
    """one of the pipeline's A/B environment switches (read when the context is created), taken down again"""
    names = []

    def put(name):
        assert name not in os.environ
        os.environ[name] = "1"
        names.append(name)
    yield put
    for n in names:
        del os.environ[n]


@pytest.mark.parametrize("name", HC.NOLLQ_CASES)
def test_ll_quantiser_of_its_own(pkg, switch, name):
    """DSV1_NO_LLQ=1: k_hz_quant<true> launches and compacts the chunks that reach into the LL region (plain, not packed)"""
    _, g, content, qp, n, labels = HC.pipe_case(name)
    switch("DSV1_NO_LLQ")
    run = HC.pipe_oracle(name)
    run_frame_by_frame(pkg, g, [run[0]], [run], dict(HC.CODING, qp=qp), name + " without llq", llq=False)


@pytest.mark.parametrize("name", HC.NOLIST_CASES)
def test_dense_pair_codes_p_pictures(pkg, switch, name):
    """DSV1_NO_LIST_PACK=1: k_hz_collect / k_hz_emit code the P pictures too"""
    _, g, content, qp, n, labels = HC.pipe_case(name)
    switch("DSV1_NO_LIST_PACK")
    run = HC.pipe_oracle(name)
    run_frame_by_frame(pkg, g, [run[0]], [run], dict(HC.CODING, qp=qp), name + " without the list kernels", list_pack=False)


def test_scan_second_tile(pkg):
    """33 streams of 2048x2080 on one coding stream, an I and a P picture each, streams alternating between clip A (entries in the
    luma plane's second tile of 2048 chunks; its P picture's first non-empty chunk there) and clip B (second tile empty): the
    256-thread k_hz_scan, once per step, walks two tiles with the carries s_c_ne, s_c_nnz and s_c_bits"""
    o = HC.tile_oracle()
    lab = {k + p["kind"]: {l for l in HC.model_of(p["planes"][0], njobs=HC.TILE_STREAMS).labels if l.startswith("sc.")} for k, r in o.items() for p in r[3]}
    assert lab == {"AI": {"sc.256", "sc.tile2.entries"}, "AP": {"sc.256", "sc.tile2.first"}, "BI": {"sc.256", "sc.tile2.empty"}, "BP": {"sc.256", "sc.tile2.empty"}}, lab
    runs = [o["AB"[s % 2]] for s in range(HC.TILE_STREAMS)]
    run_frame_by_frame(pkg, HC.TILE_G, [r[0] for r in runs], runs, dict(HC.CODING, qp=HC.TILE_QP), "tile")
