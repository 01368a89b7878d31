"""CPU checks of the inverse-transform matrix (tests/inv_cases.py) against the restated dispatch (tests/inv_plan.py).

The matrix must hold one case of every dispatch class the product has on the geometries it codes, so a new branch of
launch_inv_sbt fails here until a case is added; and together with the operator twin the cases must reach every inverse
kernel of DSVG_KERNEL_IDS but the ones listed as unreachable.  Whether the restatement is the product's dispatch is checked on
the GPU (tests/test_gpu_inv_paths.py: launches and algorithmic bytes of every inverse kernel against the plan)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import _cabi as A
import inv_cases as IC
import inv_plan as P

HOST_HPP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "digital-subband-video-1_amd", "csrc", "dsvg_host.hpp")


@functools.lru_cache(maxsize=None)
def swept():
    return P.sweep()


def inverse_kernel_ids():
    """every k_inv_* name of DSVG_KERNEL_IDS (dsvg_host.hpp)"""
    with open(HOST_HPP) as f:
        names = re.findall(r'X\(KID_\w+, "([^"]+)"\)', f.read())
    assert len(names) > 40, "DSVG_KERNEL_IDS not found"
    return {n for n in names if P.re_inverse.match(n)}


def test_matrix_covers_every_dispatch_class():
    want = swept()
    got = {}
    for g in IC.GEOMETRIES:
        got.setdefault(P.plan(*g).cls, []).append(g)
    missing = {P.describe(c): k[0] for c, k in want.items() if c not in got}
    assert not missing, "dispatch classes without a case (smallest geometry of each): %s" % missing
    extra = {P.describe(c): k for c, k in got.items() if c not in want}
    assert not extra, "cases of classes the sweep does not find: %s" % extra
    twice = {P.describe(c): k for c, k in got.items() if len(k) > 1}
    assert not twice, "classes with more than one case: %s" % twice


def test_matrix_takes_the_smallest_geometry_of_each_class():
    """(the oracle codes every one of them: no class needed its second-smallest geometry)"""
    want = swept()
    for g in IC.GEOMETRIES:
        assert want[P.plan(*g).cls][0] == g, (g, P.describe(P.plan(*g).cls))


def test_matrix_reaches_every_inverse_kernel():
    ids = inverse_kernel_ids()
    reached = set()
    for g in IC.GEOMETRIES:
        p = P.plan(*g)
        reached |= set(p.p_kernels) | set(p.i_kernels)
    assert not reached & set(P.UNREACHABLE), "listed as unreachable but planned: %s" % (reached & set(P.UNREACHABLE))
    assert reached | P.TWIN_KERNELS | set(P.UNREACHABLE) == ids, \
        "inverse kernels neither planned, nor the twin's, nor listed as unreachable: %s; unknown names: %s" % (
            ids - reached - P.TWIN_KERNELS - set(P.UNREACHABLE), (reached | P.TWIN_KERNELS | set(P.UNREACHABLE)) - ids)
    # the matrix reaches the symbol-path kernels, the twin the int32 ones: both are needed
    assert not reached <= P.TWIN_KERNELS and not P.TWIN_KERNELS <= reached


def strip_cells(g, tcx, tcy):
    """level-3 cells of the L-shaped strip launch from tile column tcx / tile row tcy on (k_sbt.hip:3494, :3517)"""
    x0, y0 = min(tcx * P.IT_TX, g.w3), min(tcy * P.IT_TY, g.h3)
    return (g.w3 - x0) * g.h3 + x0 * (g.h3 - y0)


@pytest.mark.parametrize("g", IC.GEOMETRIES, ids=IC.case_id)
def test_plan_covers_each_plane_once(g):
    """the branches of a P picture take every level-3 cell of every plane exactly once: the fast tiles or the patch kernel's
    rectangle plus the general strips; the fused border only where the patch kernel takes the chroma planes whole; one launch
    per kernel"""
    p = P.plan(*g)
    gy, gc = p.geos[0], p.geos[1]
    k = p.p_kernels
    assert all(n == 1 for n, _ in k.values()), k
    L, Ch = p.luma, p.chroma
    if L["kind"] == "fast":
        fast = min(L["fxg"] * P.IT_TX, gy.w3) * min(L["fyg"] * P.IT_TY, gy.h3)
        assert fast + strip_cells(gy, L["fxg"], L["fyg"]) == gy.w3 * gy.h3
        assert (L["nrest"] == 0) == (P.KPIX_SYM_F not in k) and P.KP_TILE_F in k
    else:
        assert set(k) & {P.KP_TILE_F, P.KPIX_SYM_F} == {P.KPIX_SYM_F}
    assert Ch["imax"] * Ch["jmax"] + strip_cells(gc, Ch["tcx"], Ch["tcy"]) == gc.w3 * gc.h3
    assert (P.KPATCH_C in k) == (Ch["imax"] * Ch["jmax"] > 0)
    assert (P.KPIX_SYM in k) == (Ch["right_strip"] or Ch["bottom_strip"])
    if Ch["part4"]:
        assert Ch["jmax"] == gc.h3 and gc.ph % 8 == 4            # the half-height last patch row stays with the patch kernel
    if Ch["fb"]:
        assert Ch["imax"] == gc.w3 and Ch["jmax"] == gc.h3 and P.KPIX_SYM not in k


def test_coarse_content_engages_the_luma_filter(orc):
    """At the coarse content's quantiser the luma smoothing filter changes pixels: the oracle's inverse transform of a forward-
    transformed frame of that content, quantised as in test_gpu_ops.test_fwd_inv_sbt, differs between the luma (c = 0,
    filtered) and the chroma (c = 1) variant."""
    c = IC.CONTENTS["coarse"]
    q = A.orc_cfg(256, 80, IC.F444, **IC.cli("coarse")).quality        # the CRF quantiser of the content's qp
    assert q > 0
    for w, h in ((144, 80), (256, 136), (32, 32)):
        clip = IC.make_content(w, h, IC.F444, "coarse", 0x7117)
        f = A.BorderedFrame(w, h, IC.F444)
        f.load_planar(clip[1])
        orc.orc_frame_extend(f.ptr())
        co = np.zeros(w * h, dtype=np.int32)
        orc.orc_fwd_sbt(C.byref(f.c.planes[0]), C.byref(A.Coefs(A.i32p(co), w, h)), 1)
        co[1:] = (co[1:] // 24) * 24
        out = []
        for cc in (0, 1):
            a = co.copy()
            fo = A.BorderedFrame(w, h, IC.F444)
            orc.orc_inv_sbt(C.byref(fo.c.planes[cc]), C.byref(A.Coefs(A.i32p(a), w, h)), q, 1, cc)
            out.append(fo.plane(cc).copy())
        assert np.count_nonzero(out[0] != out[1]) > 0, "style %d at q %d: the filter left %dx%d unchanged" % (c["style"], q, w, h)
