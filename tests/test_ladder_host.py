"""Quality ladders on the host (no GPU): the rungs' agreement check and the bounds of dsv1_ladder_open come before any device work,
and the Python Ladder checks its input size against nsources x F frames (one copy of every source, not one per rung)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _cabi as A

DSVG_ERR_ARG = -2
W, H, FMT = 176, 144, A.SUBSAMP_420


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("digital-subband-video-1_amd")


def cfg(pkg, **kw):
    return pkg.make_encoder_cfg(W, H, FMT, **dict(dict(qp=85, gop=12, rc_mode_cli=1), **kw))


def open_rc(pkg, rungs, nsources=2, F=4, device=1 << 20):
    """dsv1_ladder_open on a device number no machine has: the rungs are checked before it is looked at"""
    h = C.c_void_p(None)
    arr = (pkg.Encoder * max(len(rungs), 1))(*rungs)
    rc = pkg.lib().dsv1_ladder_open(C.byref(h), arr, len(rungs), device, nsources, F)
    assert not h.value
    return rc


def with_field(e, name, value):
    e = pkg_encoder_copy(e)
    if name.startswith("vidmeta."):
        setattr(e.vidmeta, name.split(".")[1], value)
    else:
        setattr(e, name, value)
    return e


def pkg_encoder_copy(e):
    return type(e).from_buffer_copy(e)


ANALYSIS_FIELDS = [("vidmeta.width", W + 16), ("vidmeta.height", H - 16), ("vidmeta.subsamp", A.SUBSAMP_444),
                   ("vidmeta.fps_num", 25), ("vidmeta.fps_den", 2), ("vidmeta.aspect_num", 4), ("vidmeta.aspect_den", 3),
                   ("gop", 6), ("do_scd", 0), ("scene_change_delta", 9), ("intra_pct_thresh", 30), ("stable_refresh", 5),
                   ("pyramid_levels", 3), ("rc_mode", 1)]


@pytest.mark.parametrize("field,value", ANALYSIS_FIELDS)
def test_rungs_that_disagree_on_the_analysis_are_refused(pkg, field, value):
    a = cfg(pkg)
    assert open_rc(pkg, [a, cfg(pkg, qp=40), with_field(cfg(pkg, qp=60), field, value)]) == DSVG_ERR_ARG


RATE_FIELDS = [("quality", 100), ("bitrate", 12345), ("max_q_step", 3), ("min_quality", 7), ("max_quality", 2000),
               ("min_I_frame_quality", 50), ("rc_high_motion_nudge", 0)]


@pytest.mark.parametrize("field,value", RATE_FIELDS)
def test_rungs_may_differ_in_the_rate_fields(pkg, field, value):
    """past the rung check the call reaches the device (none with this number): any failure but DSVG_ERR_ARG"""
    rc = open_rc(pkg, [cfg(pkg), with_field(cfg(pkg), field, value)])
    assert rc != DSVG_ERR_ARG and rc != 0


@pytest.mark.parametrize("nrungs", [0, -1, 17, 64])
def test_rung_count_is_bounded(pkg, nrungs):
    h = C.c_void_p(None)
    arr = (pkg.Encoder * 64)(*([cfg(pkg)] * 64))
    assert pkg.lib().dsv1_ladder_open(C.byref(h), arr, nrungs, 1 << 20, 1, 4) == DSVG_ERR_ARG


def test_rung_count_limits_pass_the_check(pkg):
    for n in (1, 16):
        rc = open_rc(pkg, [cfg(pkg)] * n)
        assert rc != DSVG_ERR_ARG and rc != 0


def test_other_arguments(pkg):
    L = pkg.lib()
    h = C.c_void_p(None)
    arr = (pkg.Encoder * 2)(cfg(pkg), cfg(pkg, qp=50))
    assert L.dsv1_ladder_open(None, arr, 2, 0, 1, 4) == DSVG_ERR_ARG
    assert L.dsv1_ladder_open(C.byref(h), None, 2, 0, 1, 4) == DSVG_ERR_ARG
    assert L.dsv1_ladder_open(C.byref(h), arr, 2, 0, 0, 4) == DSVG_ERR_ARG
    assert L.dsv1_ladder_open(C.byref(h), arr, 2, 0, 1, 0) == DSVG_ERR_ARG
    assert L.dsv1_batch_rungs(None) == DSVG_ERR_ARG


def test_python_rung_count(pkg):
    with pytest.raises(ValueError):
        pkg.Ladder([], 1, 4)
    with pytest.raises(ValueError):
        pkg.Ladder([cfg(pkg)] * 17, 1, 4)


def unopened(pkg, nsources, nrungs, F):
    """a Ladder's size bookkeeping without a device (what __init__ sets before and after dsv1_ladder_open)"""
    b = object.__new__(pkg.Ladder)
    b.h = None
    b.nsources, b.nrungs, b.F, b.nstreams = nsources, nrungs, F, nsources * nrungs
    b.frame_bytes = A.frame_bytes(W, H, FMT)
    return b


def test_python_input_size(pkg):
    S, R, F = 2, 3, 4
    b = unopened(pkg, S, R, F)
    fb = b.frame_bytes
    ok = np.zeros((S, F, fb), dtype=np.uint8)
    assert b._input(ok).size == S * F * fb
    for bad in (np.zeros((S * R, F, fb), np.uint8), np.zeros((S, F - 1, fb), np.uint8), np.zeros((S, F, fb + 1), np.uint8)):
        with pytest.raises(ValueError, match="sources"):
            b._input(bad)
        with pytest.raises(ValueError):
            b.encode(bad)
        with pytest.raises(ValueError):
            b.submit(bad)
        with pytest.raises(ValueError):
            b.stage(bad)
    assert b.stream(1, 2) == 5


def test_ladder_symbols_are_declared(pkg):
    """the new entry points are in the public header (tests/test_cabi_symbols.py checks that every declared one is exported)"""
    import test_cabi_symbols as T
    names = T.declared("dsv1_api.h")
    assert "dsv1_ladder_open" in names and "dsv1_batch_rungs" in names
