"""Every parse, position and scatter branch of the entropy decoder (csrc/k_hzcc.hip), on the GPU, against the oracle.

tests/hzdec_plan.py models the decoder's branches, tests/hzdec_cases.py lists the hand-written payloads and
tests/test_hzdec_plan_host.py proves on the CPU that they reach every label and that the model, the oracle and the reference agree.
Here the cases run on the device.  Operator seam: every case through dsvg_op_decode_plane, bit exact against orc_decode_plane; where
a plane differs the message names, through the model, the first differing entry and the chunk its value was decoded in (pass,
thread, wave, entering state, labels).  Pipeline seam: the hand-built planes spliced into real packets, through the drop-in dsv_dec
and DecBatch (host and device output), against orc_decode: an entry on the DC's cell in luma and in chroma, jobs of very unequal
payloads in one call, a call with an I and a P picture, the int32 path (DSV1_NO_DEC_SYM in a context of its own), I pictures on int32
beside P pictures on the symbol path (DSV1_NO_DEC_SYM_I), and a dense picture followed by a sparse one in one context.  The scatter
launches of every call are counted and held against the model's restatement of the launcher's decision."""
import ctypes as C
import importlib
import os

import pytest

import _cabi as A
import hzdec_cases as DC
import hzdec_plan as D
from test_gpu_stream import product_decode

pytestmark = pytest.mark.gpu

OP = DC.op_cases()


@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    L = m.lib()
    assert L.dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    L.dsvg_ctx_decoder_redone.restype = C.c_long
    L.dsvg_ctx_decoder_redone.argtypes = [C.c_void_p]
    return m


@pytest.fixture(scope="module")
def prod():
    L = A.load_prod()
    assert L.dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return L


@pytest.mark.parametrize("name", list(OP))
def test_operator_case(prod, orc, name):
    c = OP[name]
    want = DC.decode(orc, "orc_decode_plane", c)
    got = DC.decode(prod, "dsvg_op_decode_plane", c)
    if not (got == want).all():
        m = DC.model_of(name)
        raise AssertionError("%s (%dx%d, len %d of %d, %d announced): decoded plane differs from the oracle's: %s" % (
            name, c["w"], c["h"], c["len"], c["plen"], m.runs, m.explain(got, want)))


# ---------------------------------------------------------------------------------------------------------------------------
# pipeline seam
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


SCATTER = "k_hz_scatter_lv"


def run_batch(pkg, g, streams, what, sym=True, sym_i=True, want_redone=None, dropin=True):
    """streams: packet lists of equal length, one per stream of a DecBatch; every decoded frame must be the oracle's, through the
    drop-in decoder and through the batched one with host and with device output.  With host output the scatter launches of
    every call of pictures are counted by the context's kernel profiler and must be the model's (scatter_launches): three show
    that planes of the call kept int32 coefficients, one that none did.  (A call that is decoded again adds its launches to a
    later call's count, so the counts are held against the model where nothing was redone)"""
    w, h, fmt = g
    L = pkg.lib()
    want = [A.orc_decode(b"".join(pk), w, h, fmt) for pk in streams]
    assert all(len(pk) == len(streams[0]) for pk in streams)
    if dropin:
        for s, pk in enumerate(streams):
            got = product_decode(pkg, b"".join(pk))
            assert len(got) == len(want[s])
            for t in range(len(got)):
                A.assert_same("%s: dsv_dec stream %d frame %d" % (what, s, t), got[t], want[s][t])
    names = [L.dsvg_prof_kernel_name(i).decode() for i in range(L.dsvg_prof_kernels())]
    kid = names.index(SCATTER)
    for on_device in (False, True):
        d = pkg.DecBatch(w, h, fmt, len(streams))
        try:
            if not on_device:
                A.chk(L, L.dsvg_prof_enable(d.ctx, 1 << kid))
            k = [0] * len(streams)
            launched, model = [], []
            for ps in zip(*streams):
                if not on_device:
                    A.chk(L, L.dsvg_prof_reset(d.ctx))
                out, status, fnum = d.decode(list(ps), on_device=on_device)
                frames = None
                kinds = ""
                for s, p in enumerate(ps):
                    if status[s] == 0 and (p[5] & 4):
                        kinds += "P" if p[5] & 1 else "I"
                        if frames is None:
                            frames = d.download() if on_device else out
                        A.assert_same("%s: batched decoder (device output %s) stream %d frame %d" % (what, on_device, s, k[s]), frames[s], want[s][k[s]])
                        k[s] += 1
                if kinds and not on_device:
                    ms, n, by = C.c_double(0), C.c_long(0), C.c_double(0)
                    A.chk(L, L.dsvg_prof_get(d.ctx, kid, C.byref(ms), C.byref(n), C.byref(by)))
                    launched.append((kinds, n.value))
                    model.append((kinds, D.scatter_launches(kinds, sym, sym_i)))
            assert k == [len(x) for x in want], k
            redone = L.dsvg_ctx_decoder_redone(d.ctx)
            if want_redone is not None:
                assert (redone >= 1) == want_redone, "%s: calls decoded again from int32 coefficients: %d" % (what, redone)
            if not on_device and redone == 0:
                assert launched == model, "%s: %s launches per call %s, the model says %s" % (what, SCATTER, launched, model)
        finally:
            d.close()


@pytest.mark.parametrize("plane", [0, 1])
def test_entry_on_the_dc_cell(pkg, orc, plane):
    """a first run of 0 puts entry 1 on the DC's cell: the reference writes it and then the DC over it (hzcc.c:340, 495).  The DC is
    one every sample of the decoded plane depends on (tests/test_hzdec_plan_host.py shows it): were entry 1's symbol to win the
    cell, the frame would differ.  Nothing in the plane for the symbol path to escape from"""
    call = DC.PIPE_CALLS["pos0-luma" if plane == 0 else "pos0-chroma"]
    assert "sc.pos0" in D.Plane(**{k: call["planes"][0][k] for k in ("w", "h", "buf")}, length=call["planes"][0]["plen"]).labels
    pk = DC.spliced(DC.PIPE_G, "IP", DC.POS0_SEED, [(1, plane, "pos0")])
    run_batch(pkg, DC.PIPE_G, [pk, pk], "entry on the DC's cell, plane %d" % plane, want_redone=False)


@pytest.mark.parametrize("sym", [True, False])
def test_unequal_jobs_in_one_call(pkg, orc, switch, sym):
    """a plane without entries beside a three-pass plane in one call of P pictures: the grids are sized by the large job"""
    call = DC.PIPE_CALLS["unequal" if sym else "unequal-i32"]
    assert "la.unequal" in D.call_labels(call["kinds"], sym, call["lens"])
    if not sym:
        switch("DSV1_NO_DEC_SYM")
    a = DC.spliced(DC.PIPE_G, "IP", 0xDEC1, [(1, 0, "empty")])
    b = DC.spliced(DC.PIPE_G, "IP", 0xDEC1, [(1, 0, "three-pass")])
    run_batch(pkg, DC.PIPE_G, [a, b], "unequal jobs (%s)" % ("symbol path" if sym else "int32 path"), sym=sym, want_redone=None if sym else False, dropin=sym)


@pytest.mark.parametrize("path", ["sym", "i32", "mixed"])
def test_call_with_an_i_and_a_p_picture(pkg, orc, switch, path):
    """one scatter launch while the I picture is on the symbol path too; three under DSV1_NO_DEC_SYM (every plane int32) and under
    DSV1_NO_DEC_SYM_I, where the first launch serves the P picture's symbol planes and level group 0 of the I picture's int32
    planes in one grid and the two that follow skip the symbol planes"""
    call = DC.PIPE_CALLS[{"sym": "i-and-p", "i32": "i-and-p-i32", "mixed": "i-and-p-mixed"}[path]]
    sym, sym_i = call["sym"], call.get("sym_i", True)
    if path != "sym":
        switch("DSV1_NO_DEC_SYM" if path == "i32" else "DSV1_NO_DEC_SYM_I")
    a = DC.spliced(DC.PIPE_G, "IP", 0xDEC2, [(1, 2, "pos0")])
    b = DC.spliced(DC.PIPE_G, "II", 0xDEC2, [(1, 0, "sparse"), (1, 1, "pos0")])
    assert len(b) == len(a) + 1 and not (b[2][5] & 4), "a GOP of one repeats the stream's metadata before its second picture"
    a.insert(2, a[0])                                     # ... so the other stream repeats its own there: the calls stay aligned
    assert set(call["labels"]) <= D.call_labels("PI", sym, None, sym_i)
    run_batch(pkg, DC.PIPE_G, [a, b], "I and P in one call (%s)" % path, sym=sym, sym_i=sym_i, want_redone=False if path != "sym" else None, dropin=path == "sym")


def test_dense_then_sparse_in_one_context(pkg, orc):
    """what k_hz_unscatter or k_dec_clear leaves behind of the dense picture would show in the sparse one after it"""
    pk = DC.spliced(DC.PIPE_G, "IPP", 0xDEC3, [(1, 0, "three-pass"), (1, 1, "three-pass"), (2, 0, "sparse"), (2, 1, "empty")])
    run_batch(pkg, DC.PIPE_G, [pk], "dense then sparse")
