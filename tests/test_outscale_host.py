"""Decoder output scale, what can be said without a GPU: the new calls are declared and exported, a NULL handle is refused before any
device is touched, and the target lists of tests/test_gpu_outscale.py (tests/outscale_cases.py) pass or fail the numpy definition's
per-plane ratio rule -- and the library's own host-side tap count -- exactly where the GPU tests expect a refusal."""
import ctypes as C
import os

import pytest

import _cabi as A
import _resample as RS
import outscale_cases as OC
from test_cabi_symbols import declared

DSVG_ERR_ARG = -2
NEW = {"dsvg.h": ["dsvg_ctx_output_scale"], "dsv1_api.h": ["dsv1_decbatch_set_output_scale", "dsv1_decbatch_out_dims"]}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(A.PROD_SO):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(A.PROD_SO)


@pytest.mark.parametrize("header", sorted(NEW))
def test_the_new_calls_are_declared_and_exported(lib, header):
    names = declared(header)
    for n in NEW[header]:
        assert n in names, "%s is not declared in include/%s" % (n, header)
        assert hasattr(lib, n), "%s is declared but not exported" % n


def test_null_handles_are_refused_without_a_device(lib):
    lib.dsv1_decbatch_set_output_scale.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.dsv1_decbatch_out_dims.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.dsvg_ctx_output_scale.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    w, h = C.c_int(-7), C.c_int(-7)
    for args in ((176, 144, RS.CUBIC), (0, 0, RS.TENT), (176, 144, 9)):
        assert lib.dsv1_decbatch_set_output_scale(None, *args) == DSVG_ERR_ARG
        assert lib.dsvg_ctx_output_scale(None, *args) == DSVG_ERR_ARG
    assert lib.dsv1_decbatch_out_dims(None, C.byref(w), C.byref(h)) == DSVG_ERR_ARG
    assert (w.value, h.value) == (-7, -7)


def all_targets():
    for table, ok in ((OC.CTX_TARGETS, True), (OC.DEC_TARGETS, True), (OC.ACCEPTED_EDGE, True), (OC.REFUSED, False)):
        for (sw, sh, fmt), targets in sorted(table.items()):
            for dw, dh in targets:
                yield sw, sh, fmt, dw, dh, ok


def test_the_target_lists_meet_the_definitions_ratio_rule(lib):
    """accepted targets build their tables in numpy (weights() asserts the rule); refused ones trip that assertion on some plane; the
    library's host-side dsv1_resample_taps agrees plane by plane"""
    lib.dsv1_resample_taps.argtypes = [C.c_int] * 3
    seen = {True: 0, False: 0}
    for sw, sh, fmt, dw, dh, ok in all_targets():
        assert OC.ratio_ok(sw, sh, fmt, dw, dh) == ok, (sw, sh, fmt, dw, dh)
        seen[ok] += 1
        if dw < 1 or dh < 1:
            continue
        fails = 0
        for (pw, ph), (qw, qh) in zip(OC.plane_dims(sw, sh, fmt), OC.plane_dims(dw, dh, fmt)):
            for S, D in ((pw, qw), (ph, qh)):
                for filt in (RS.TENT, RS.CUBIC):
                    try:
                        RS.weights(S, D, filt)
                        assert lib.dsv1_resample_taps(S, D, filt) == RS.taps(S, D, filt), (S, D, filt)
                    except AssertionError:
                        assert not (S <= 8 * D and D <= 8 * S), (S, D)
                        assert lib.dsv1_resample_taps(S, D, filt) < 0, (S, D, filt)
                        fails += 1
        assert (fails == 0) == ok, (sw, sh, fmt, dw, dh)
    assert seen[True] >= 15 and seen[False] >= 8


def test_the_lists_hold_the_cases_they_are_there_for():
    S420, S422, S444 = OC.S420, OC.S422, OC.S444
    t = OC.CTX_TARGETS[(250, 130, S420)]
    assert (125, 65) in t and (63, 17) in t and (500, 260) in t and (333, 40) in t and (250, 130) in t
    assert 63 % 4 == 3 and 7 < 130 / 17 <= 8                       # the byte stores of a row's last quad; ratio near 8 on the height
    assert A.chroma_dims(250, 130, S420) == (125, 65) and A.chroma_dims(125, 65, S420) == (63, 33)
    assert OC.DEC_TARGETS[(352, 288, S420)] == [(176, 144), (44, 36), (704, 576)]
    assert OC.DEC_TARGETS[(360, 200, S422)] == [(45, 25), (641, 75)]
    assert OC.DEC_TARGETS[(320, 240, S444)] == [(321, 239), (100, 36)]
    for (pw, ph), (qw, qh) in zip(OC.plane_dims(352, 288, S420), OC.plane_dims(44, 36, S420)):
        assert pw == 8 * qw and ph == 8 * qh                         # ratio 8 on every plane
    assert (43, 36) in OC.REFUSED[(352, 288, S420)] and (2817, 288) in OC.REFUSED[(352, 288, S420)] and 8 * 352 == 2816
